"""
Training loop for QuanONetPT / HEAQNNPT on the HIP quantum layer: host-side mirror of the
reference's ``solvers/solver_pt.py`` (PTSolver) plus the data-parallel step the reference lacks.

* ``DataParallelTrainer``: one training step = forward -> MSE -> in-kernel adjoint backward ->
  ONE sum over the ranks of a flat fp64 buffer [all gradients | sse | sum y^2] -> Adam (``PeerExchange``: both in
  one kernel over peer-mapped buffers; ``dist.all_reduce`` + an Adam launch where that is not available).
  Each rank's loss is ``sum((pred-y)^2) / global_batch`` so that a plain SUM reproduces the
  gradient of ``MSELoss(mean)`` over the global batch (solver_pt.py:232-236), also for uneven
  shards.  The two logging scalars ride in the same buffer, removing the reference's two
  ``.item()`` host syncs per batch (solver_pt.py:238-241).
* ``PTSolver``: config-dict driven epoch/batch loop with the reference's semantics
  (solver_pt.py:191-329): ``np.random.permutation`` batch order, best-by-train-loss checkpoint
  as ``.pt`` + ``.npz`` with the reference's state_dict keys, final checkpoint, evaluate() with
  rel-L2 / MSE / MAE / max-error.  Training data stay resident on the device.
"""
import collections
import json
import os
import random

import numpy as np
import torch
import torch.nn as nn


def set_random_seed(seed):
    """
    What the reference's launcher does before it builds the solver (utils/common.py:154-180, main.py): seed
    ``random``, NumPy's global generator (the per-epoch ``np.random.permutation``, solver_pt.py:220) and torch (the
    U(-pi,pi) draw of the circuit weights, core/quantum_circuits_tq.py:50-53).  PTSolver itself never seeds, exactly
    like the reference's; in a multi-rank run only rank 0's NumPy state matters (it draws, the others receive).
    """
    if seed is None:
        return
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def shard_slice(n_items, rank, world):
    """Contiguous, near-even shard [lo, hi) of a batch of n_items for `rank` of `world`."""
    base, rem = divmod(n_items, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def split_inputs(inputs):
    """(branch, trunk or None) of a model's input tuple: (branch, trunk) for QuanONet, (x,) for HEAQNN"""
    return inputs[0], (inputs[1] if len(inputs) > 1 else None)


def run_dir(config):
    """The directory PTSolver(config) writes its checkpoints and metric.json to."""
    return os.path.join(config.get('prefix') or 'outputs', config.get('operator', 'Op'), config.get('run_id', 'run'))


# the model settings a config may leave out, and how a given value is read (PTSolver._create_model and the member validators)
_MODEL_DEFAULTS = {'net_size': [20, 2, 10, 2], 'if_trainable_freq': 'true', 'scale_coeff': 0.01, 'ham_bound': [-5, 5]}
_MODEL_PARSE = {'net_size': tuple, 'if_trainable_freq': lambda v: str(v).lower() == 'true', 'scale_coeff': float,
                'ham_bound': tuple}


def model_setting(config, key):
    """config[key] as the model takes it, PTSolver's default where the config leaves it out"""
    return _MODEL_PARSE[key](config.get(key, _MODEL_DEFAULTS[key]))


def batch_plan(n, bs):
    """(number of steps, global batch of each step, row bounds of the steps in an epoch's n gathered rows)"""
    nb = max(1, int(np.ceil(n / bs)))
    return nb, [min(bs, n - i * bs) for i in range(nb)], [min(i * bs, n) for i in range(nb)] + [n]


def epoch_sums(tl, gbs):
    """(mean batch MSE, sse, sum y^2, the steps' MSE) of one epoch from its [sse, sum y^2] rows, added in step order"""
    step_mse = [t[0] / gb for t, gb in zip(tl, gbs)]
    s = [0.0, 0.0, 0.0]
    for t, mse in zip(tl, step_mse):
        s[0] += mse
        s[1] += t[0]
        s[2] += t[1]
    return s[0] / len(gbs), s[1], s[2], step_mse


def run_epochs(epochs, first, stage, issue, check_status, snapshot, schedulers, record):
    """
    The epoch loop of PTSolver.train and EnsembleSolver.train, one epoch ahead of its bookkeeping.  `first`: the staged first
    epoch; stage() draws the next epoch's order and gathers its rows; issue(staged) queues an epoch's steps and returns (the
    device rows of its [sse | sum y^2], whatever snapshot needs of it); snapshot(that) copies to the host what the bookkeeping
    needs from the END of the epoch (the parameters for the checkpoint); record(epoch, tails as lists, snapshot) does the sums,
    the checkpoint and the log line.
    """
    cur = issue(first) if epochs > 0 else None
    for epoch in range(epochs):
        tails, extra = cur
        # the next epoch's order and rows are drawn and gathered BEFORE the host waits for this epoch: the draw (a
        # millisecond of host time at 10^5 rows) overlaps the steps still queued on the device
        staged = stage() if epoch + 1 < epochs else None
        tl = tails.tolist()                                 # one host sync per epoch
        check_status()                                      # a kernel-side pipeline failure ends the run here
        # What the bookkeeping needs from the END of this epoch is on the host after the snapshot -- the losses, and (19 KB)
        # the parameters for the best-by-train-loss checkpoint -- so the NEXT epoch is queued first and the host does its
        # sums, its checkpoint and its log line while the device already works (the schedulers offered are functions
        # of the epoch count alone).
        snap = snapshot(extra)
        for sched in schedulers:
            sched.step()
        cur = issue(staged) if staged is not None else None
        record(epoch, tl, snap)


def regression_metrics(y_pred, y_true, dist=None, world=1):
    """
    MSE / MAE / Max_Error (utils/metrics.py:6-29) and relative L2 (solvers/solver_pt.py:316-321) of a test set that is
    sharded over `world` ranks: every rank passes ITS slice of predictions and targets (torch tensors, any device);
    four sums and one maximum are all-reduced, so every rank returns the metrics of the whole set.
    """
    d = (y_pred.reshape(-1) - y_true.reshape(-1)).to(torch.float64)
    yt = y_true.reshape(-1).to(torch.float64)
    sums = torch.stack([(d * d).sum(), d.abs().sum(), (yt * yt).sum(),
                        torch.tensor(float(d.numel()), dtype=torch.float64, device=d.device)])
    mx = d.abs().max() if d.numel() else torch.zeros((), dtype=torch.float64, device=d.device)
    mx = mx.reshape(1)
    if dist is not None and world > 1:
        dist.all_reduce(sums)
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
    sse, sae, sy2, cnt = sums.tolist()
    return {'MSE': sse / cnt, 'MAE': sae / cnt, 'Max_Error': float(mx.item()),
            'rel_l2': float(np.sqrt(sse) / (np.sqrt(sy2) + 1e-8))}


class FlatAdam(torch.optim.Optimizer):
    """
    torch.optim.Adam arithmetic (amsgrad=False) on the trainer's flat fp64 vector through ``qhea_adam_step``:
    one launch per update instead of torch's two multi-tensor kernels.  A regular ``Optimizer`` (param_groups,
    lr schedulers, state_dict) so that PTSolver's scheduler handling is unchanged.
    """

    def __init__(self, params, pflat, gflat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(list(params), dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.pflat, self.gflat = pflat, gflat
        self.exp_avg = torch.zeros_like(pflat)
        self.exp_avg_sq = torch.zeros_like(pflat)
        self.t = 0

    def hparams(self):
        """(lr, beta1, beta2, eps, weight_decay) of the param group: the tail of every _lib call with an Adam update"""
        g = self.param_groups[0]
        return g['lr'], g['betas'][0], g['betas'][1], g['eps'], g['weight_decay']

    @torch.no_grad()
    def step(self, closure=None):
        from . import _lib
        self.t += 1
        _lib.adam_step(self.pflat, self.gflat, self.exp_avg, self.exp_avg_sq, self.t, *self.hparams())

    def state_dict(self):
        sd = super().state_dict()
        sd['flat_state'] = {'step': self.t, 'exp_avg': self.exp_avg.clone(), 'exp_avg_sq': self.exp_avg_sq.clone()}
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)
        fs = sd.pop('flat_state', None)
        super().load_state_dict(sd)
        if fs is not None:
            self.t = int(fs['step'])
            self.exp_avg.copy_(fs['exp_avg'])
            self.exp_avg_sq.copy_(fs['exp_avg_sq'])


class PeerExchange:
    """
    The data-parallel step's gradient sum + Adam update as ONE kernel per rank over peer-mapped exchange buffers
    (include/quanonet_hea.h: qhea_dp_*, csrc/hea_dp.hip) instead of ``dist.all_reduce`` + a separate Adam launch.

    Set-up uses the process group only for hand-shakes: the 64-byte hipIpc handles travel by ``all_gather_object``,
    every rank maps the others' buffers, and a three-round self-check (both slot parities, slot reuse) is compared with
    the analytic sum.  ``create`` returns None -- on EVERY rank, the outcome is agreed by an all-reduce -- when any
    rank could not map a buffer or saw a wrong sum; the trainer then keeps the RCCL all-reduce.  ``QHEA_DP_EXCHANGE=rccl``
    switches the peer path off.
    """

    def __init__(self, dist, rank, world, n_values, device, timeout_ms=5000.0):
        self.dist, self.rank, self.world, self.n, self.device = dist, rank, world, int(n_values), device
        self.timeout_ms = float(timeout_ms)
        self.seq = 0
        self.own = None
        self.bufs = [None] * world

    @classmethod
    def create(cls, dist, rank, world, n_values, device, log=None):
        """Returns (exchange or None, reason): the reason says in words which path the data-parallel step takes and why
        (bench.py prints it as config.dp_exchange_reason; rank 0 logs it)."""
        from . import _lib
        say = log if (log is not None and rank == 0) else (lambda *a, **k: None)

        def out(px, reason):
            say("data-parallel exchange: " + reason)
            return px, reason
        if world < 2:
            return None, "single rank: no exchange"
        if world > _lib.DP_MAX_RANKS or device.type != 'cuda':
            return out(None, f"all_reduce: world size {world} on {device.type} is outside the peer exchange "
                             f"(HIP devices, at most {_lib.DP_MAX_RANKS} ranks)")
        if os.environ.get('QHEA_DP_EXCHANGE', 'peer').lower() in ('rccl', 'nccl', 'off', '0'):
            return out(None, "all_reduce: QHEA_DP_EXCHANGE=" + os.environ['QHEA_DP_EXCHANGE'])
        env = os.environ.get(_lib.IPC_ENV)
        env_note = ""
        if env != '0':
            env_note = f" ({_lib.IPC_ENV}={env!r}: hipIpc handles need the dmabuf mode, value 0)"
        elif _lib.IPC_ENV_SET_LATE:
            env_note = f" ({_lib.IPC_ENV}=0 was set after this process had initialised the GPU: export it before launch)"
        self = cls(dist, rank, world, n_values, device)
        ok, why = 1, ""
        handle = None
        try:
            self.own = _lib.dp_alloc(self.n, world, device)
            handle = _lib.dp_export(self.own, device)
        except _lib.QheaError as e:
            ok, why = 0, f"rank {rank}: {e}"
        handles = [None] * world
        dist.all_gather_object(handles, handle)
        if ok and all(h is not None for h in handles):
            self.bufs[rank] = self.own
            try:
                for r in range(world):
                    if r != rank:
                        self.bufs[r] = _lib.dp_import(handles[r], device)
            except _lib.QheaError as e:
                ok, why = 0, f"rank {rank}: {e}"
        elif ok:
            ok, why = 0, "a peer could not allocate or export its buffer"
        whys = [None] * world
        dist.all_gather_object(whys, why)                      # everybody learns the first failure's text
        if not self._agree(ok):
            self.close()
            first = next((w for w in whys if w), "unknown")
            return out(None, f"all_reduce: peer buffers could not be mapped on every rank [{first}]{env_note}")
        if not self._agree(self._self_check()):
            self.close()
            return out(None, f"all_reduce: the peer exchange's self-check (three rounds against the analytic sum) failed{env_note}")
        return out(self, f"peer-mapped buffers over hipIpc, {world} ranks, {self.n} values per rank; self-check passed")

    def _agree(self, ok):
        t = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device=self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN)
        return bool(t.item() > 0.5)

    def _self_check(self):
        from . import _lib
        good = True
        base = torch.arange(1, self.n + 1, dtype=torch.float64, device=self.device) * 1e-3
        for rnd in range(3):
            local = base * (self.rank + 1) + rnd
            out = torch.empty_like(local)
            self.seq += 1
            _lib.dp_allreduce_adam(self.rank, self.world, self.bufs, self.seq, local, out, timeout_ms=2000.0)
            try:
                _lib.dp_status(self.own, self.device)
            except _lib.QheaError:
                good = False
            want = base * (self.world * (self.world + 1) / 2) + rnd * self.world
            good = good and bool(torch.allclose(out, want, rtol=1e-13, atol=0.0))
        return good

    def allreduce_adam(self, flat, pflat, opt):
        """flat <- sum over ranks of flat (rank order); FlatAdam `opt`'s update of pflat with it; one launch."""
        from . import _lib
        opt.t += 1
        self.seq += 1
        _lib.dp_allreduce_adam(self.rank, self.world, self.bufs, self.seq, flat, flat, pflat, opt.exp_avg,
                               opt.exp_avg_sq, opt.t, *opt.hparams(), timeout_ms=self.timeout_ms)

    def check_status(self):
        from . import _lib
        _lib.dp_status(self.own, self.device)

    def close(self):
        """Collective: every rank calls it (also the ranks whose own allocation failed in create)."""
        from . import _lib
        for r, b in enumerate(self.bufs):
            if b is not None and r != self.rank:
                try:
                    _lib.dp_close(b, self.device)
                except _lib.QheaError:
                    pass
        self.bufs = [None] * self.world
        self.dist.barrier()                            # every importer has closed its mapping of the buffers freed next
        if self.own is not None:
            _lib.dp_free(self.own, self.device)
            self.own = None


def _train_noise(v):
    """config value / argument `train_noise` -> NoiseModel or None (a NoiseModel, or a dict of its fields)"""
    if v is None:
        return None
    from .noise import _GRADIENT_WHY, NoiseModel, _uniform_only
    if isinstance(v, NoiseModel):
        return v
    _uniform_only(v, 'train_noise', _GRADIENT_WHY)
    if isinstance(v, dict):
        return NoiseModel(**v)
    raise ValueError(f"train_noise must be a quanonet_amd.noise.NoiseModel or a dict of its fields (got {type(v).__name__})")


def _train_device_noise(v, train_noise=None):
    """config value / argument `train_device_noise` -> DeviceNoise or None (a DeviceNoise, or its asdict() form); a key of its
    own because the dict forms of the two noise records have different fields.  Both keys together are refused."""
    if v is None:
        return None
    from .noise import DeviceNoise
    if train_noise is not None:
        raise ValueError("train_noise and train_device_noise are both set: a run trains under one noise model")
    if isinstance(v, DeviceNoise):
        return v
    if isinstance(v, dict):
        return DeviceNoise.fromdict(v)
    raise ValueError("train_device_noise must be a quanonet_amd.noise.DeviceNoise or its asdict() form "
                     f"(got {type(v).__name__}); a NoiseModel goes to train_noise")


def _train_noise_states(v, train_noise=None, train_device_noise=None, sampling_keys=()):
    """config value / argument `train_noise_states` -> 'inverse' (the default: rho walked back through the inverse channels) or
    'stored' (rho replayed from the states the forward sweep stored, qhea_model_train_steps_noisy_device_exact_stored).
    `sampling_keys`: the sampling keys that are set.  'stored' belongs to the exact loss under train_device_noise alone."""
    if v is None or v == 'inverse':
        return 'inverse'
    if v != 'stored':
        raise ValueError(f"train_noise_states must be 'inverse' (rho walked back through the inverse channels, the default) or "
                         f"'stored' (rho replayed from stored forward states) (got {v!r})")
    if train_noise is not None:
        raise ValueError("train_noise_states='stored' does not combine with train_noise: under a uniform NoiseModel every "
                         "gradient entry shrinks by the amplification the guard bounds, so past the guard there is nothing left "
                         "to train; stored states are the walk of train_device_noise")
    for key in sampling_keys:
        raise ValueError(f"train_noise_states='stored' does not combine with {key}: a sampled-trajectory gradient walks pure "
                         "states back through unitaries and has no inverse channel to replace; stored states belong to the "
                         "exact loss of train_device_noise alone (n <= 6)")
    if train_device_noise is None:
        raise ValueError("train_noise_states='stored' needs train_device_noise: it says how the exact gradient under that "
                         "DeviceNoise carries rho back")
    return 'stored'


def _train_noise_exact(v, train_noise=None, other_keys=()):
    """config value / argument `train_noise_exact` -> None (train_noise alone trains on the exact loss at n <= 6 and refuses
    beyond) or 'wide' (the exact noisy loss for every n it exists for: n <= 6 as train_noise alone, n = 7..9 on tiles)"""
    if v is None:
        return None
    if v != 'wide':
        raise ValueError(f"train_noise_exact must be None or 'wide' (the exact noisy loss for n = 2..9; got {v!r})")
    if other_keys:
        raise ValueError(f"train_noise_exact='wide' does not combine with {other_keys[0]}: it asks for the exact loss under the "
                         "NoiseModel of train_noise, neither a sampled loss nor a DeviceNoise")
    if train_noise is None:
        raise ValueError("train_noise_exact='wide' needs train_noise: it says which calls differentiate the exact loss under "
                         "that NoiseModel")
    return v


def _train_device_noise_exact(v, train_device_noise=None, other_keys=(), train_noise_states=None):
    """config value / argument `train_device_noise_exact` -> None (train_device_noise alone trains on the exact loss at n <= 6
    and refuses beyond), 'wide' (the exact loss under the DeviceNoise for every n it exists for: n <= 6 as train_device_noise
    alone, n = 7..9 on tiles, rho walked back through the inverse channels) or 'stored' (the same loss with rho replayed from
    stored states at every n it exists for: n <= 6 as train_device_noise with train_noise_states='stored', n = 7..9 on tiles).
    `other_keys`: the keys set beside it that it does not combine with."""
    if v is None:
        return None
    if v not in ('wide', 'stored'):
        raise ValueError(f"train_device_noise_exact must be None or 'wide' (the exact device-noisy loss for n = 2..9), or 'stored' "
                         f"(that loss with rho replayed from stored states, n = 2..9; got {v!r})")
    if other_keys:
        raise ValueError(f"train_device_noise_exact={v!r} does not combine with {other_keys[0]}: it asks for the exact loss "
                         "under the DeviceNoise of train_device_noise, neither a uniform NoiseModel nor a sampled loss")
    if train_device_noise is None:
        raise ValueError(f"train_device_noise_exact={v!r} needs train_device_noise: it says which calls differentiate the exact "
                         "loss under that DeviceNoise")
    if v == 'stored' and train_noise_states not in (None, 'stored'):
        raise ValueError(f"train_device_noise_exact='stored' replays rho from stored states: train_noise_states beside it is "
                         f"absent or 'stored' (got {train_noise_states!r})")
    return v


def _train_sampling(v, key='train_sampling'):
    """config value / argument `train_sampling` or `train_trajectories` -> Sampling or None (a Sampling, or its asdict() form)"""
    if v is None:
        return None
    from .noise import Sampling
    if isinstance(v, Sampling):
        return v
    if isinstance(v, dict):
        return Sampling(**v)
    raise ValueError(f"{key} must be a quanonet_amd.noise.Sampling or its asdict() form (got {type(v).__name__})")


# The loss a DataParallelTrainer trains on, chosen once in __init__ by one function per family (_ideal_loss, _exact_loss,
# _exact_wide_loss, _exact_device_loss, _exact_device_wide_loss, _sampled_loss, _jump_loss):
#   loss_grad(data, inv, grad, step, row0, ham_diag)    behind loss_and_grad; data = (desc, branch, trunk, y, params), step the
#                                                       Adam count of the update the gradient is for, row0 its first global row
#   steps(call, ham_diag)                               behind _steps; call = a steps entry's arguments up to weight_decay
#   single                                              one train_step on a single device: 'loss_grad+adam' (loss_grad under the
#                                                       step's record, then the Adam launch), 'steps' (one step of the steps
#                                                       entry) or 'train_step' (model_train_step)
#   step_record(step)                                   the record of a sampled loss with seed + step (mod 2^64), or None: `step`
#                                                       = 0 is the record the steps entry takes (it adds the step count itself)
TrainLoss = collections.namedtuple('TrainLoss', 'loss_grad steps single step_record')


def _exact_train_loss(loss_grad, steps, record):
    """an exact noisy loss: its two calls with record() behind the data; the steps entry is its only fused step"""
    return TrainLoss(lambda data, inv, grad, step, row0, ham_diag: loss_grad(*data, record(), inv, grad, ham_diag=ham_diag),
                     lambda call, ham_diag: steps(*call, record(), ham_diag=ham_diag), 'steps', None)


def _sampled_train_loss(loss_grad, steps, step_record):
    """a sampled loss: its two calls with the step's record behind the data.  The steps entry reads a step's global rows off its
    schedule; one step with rows of its own is the loop the entry is bitwise equal to: the single call under seed + step count,
    then the Adam launch"""
    return TrainLoss(lambda data, inv, grad, step, row0, ham_diag: loss_grad(*data, step_record(step), inv, grad, row0=row0,
                                                                             ham_diag=ham_diag),
                     lambda call, ham_diag: steps(*call, step_record(0), ham_diag=ham_diag), 'loss_grad+adam', step_record)


class DataParallelTrainer:
    """
    fused='auto': when the model is one of this package's QuanONetPT / HEAQNNPT (fp64, on a HIP
    device) the step runs through the model-level C ABI (qhea_model_loss_grad: three launches);
    otherwise through torch autograd on the module (HEACircuitHIP's autograd.Function).  Both paths
    fill the same flat buffer, so the collective and the optimizer step are shared.
    """

    def __init__(self, model, lr=1e-4, world_size=1, dist=None, optimizer='adam', optimizer_kwargs=None,
                 fused='auto', peer_exchange=True, log=None, train_noise=None, train_device_noise=None,
                 train_sampling=None, train_trajectories=None, train_jump_trajectories=None, train_noise_states=None,
                 train_noise_exact=None, train_device_noise_exact=None):
        self.model = model
        self.train_noise = _train_noise(train_noise)
        self.train_noise_exact = _train_noise_exact(
            train_noise_exact, self.train_noise,
            [k for k, v in (('train_device_noise', train_device_noise), ('train_sampling', train_sampling),
                            ('train_trajectories', train_trajectories), ('train_jump_trajectories', train_jump_trajectories),
                            ('train_noise_states', train_noise_states)) if v is not None])
        self.train_device_noise = _train_device_noise(train_device_noise, train_noise)
        self.noise_states = _train_noise_states(
            train_noise_states, self.train_noise, self.train_device_noise,
            [k for k, v in (('train_sampling', train_sampling), ('train_trajectories', train_trajectories),
                            ('train_jump_trajectories', train_jump_trajectories)) if v is not None])
        self.train_device_noise_exact = _train_device_noise_exact(
            train_device_noise_exact, self.train_device_noise,
            [k for k, v in (('train_noise', train_noise), ('train_sampling', train_sampling),
                            ('train_trajectories', train_trajectories), ('train_jump_trajectories', train_jump_trajectories))
             if v is not None], train_noise_states)
        if self.train_device_noise_exact == 'stored':
            self.noise_states = 'stored'
        # train_jump_trajectories beside train_device_noise: what train_trajectories means there, for every n a quantum-jump
        # gradient exists for (7..12); train_trajectories there keeps the range it was introduced with (7..9)
        if train_jump_trajectories is not None:
            if train_trajectories is not None or train_sampling is not None:
                other = 'train_trajectories' if train_trajectories is not None else 'train_sampling'
                raise ValueError(f"train_jump_trajectories and {other} are both set: set one of them (beside train_device_noise "
                                 "train_jump_trajectories covers n = 7..12, train_trajectories n = 7..9)")
            if self.train_device_noise is None:
                raise ValueError("train_jump_trajectories needs train_device_noise: it says how the DeviceNoise of "
                                 "train_device_noise is sampled (quantum-jump trajectories, n = 7..12); train_trajectories is "
                                 "the key beside train_noise")
        # Two keys, one meaning: train_sampling keeps the range it was introduced with (n = 7..9, and its refusal beyond),
        # train_trajectories is the same request for every n a sampled gradient exists for (7..12).  self.train_sampling is the
        # Sampling in force under either key, self.sampling_key the key it came by.
        if train_sampling is not None and train_trajectories is not None:
            raise ValueError("train_sampling and train_trajectories say the same thing: set one of them (train_trajectories "
                             "covers n = 7..12, train_sampling n = 7..9)")
        self.sampling_key = key = ('train_jump_trajectories' if train_jump_trajectories is not None else
                                   'train_sampling' if train_trajectories is None else 'train_trajectories')
        self.train_sampling = _train_sampling(train_jump_trajectories if train_jump_trajectories is not None else
                                              train_sampling if train_trajectories is None else train_trajectories, key)
        if self.train_sampling is not None:
            # sampled-trajectory training (qhea_model_train_steps_noisy_wide / _lds): what it cannot combine with
            # ... or quantum-jump training under a device model (qhea_model_train_steps_noisy_device): train_trajectories beside
            # train_device_noise
            if self.train_device_noise is not None and key == 'train_sampling':
                raise ValueError("train_sampling does not combine with train_device_noise: train_trajectories is the key that "
                                 "says how the DeviceNoise of train_device_noise is sampled (quantum-jump trajectories, "
                                 "n = 7..9; train_jump_trajectories: n = 7..12)")
            if self.train_device_noise is None and self.train_noise is None:
                raise ValueError(f"{key} needs train_noise: it says how the NoiseModel of train_noise is sampled")
            if self.train_sampling.shots > 0:
                raise ValueError(f"{key}: training differentiates expectation mode (Sampling.shots = 0, trajectories "
                                 "= T); a sampled bitstring has no gradient")
            if int(world_size) > 1:
                raise ValueError(f"{key}: sampled-trajectory training runs on one device (world_size = 1)")
        self.world = int(world_size)
        self.dist = dist
        self.params = [p for p in model.parameters() if p.requires_grad]
        p0 = self.params[0]
        self.numel = sum(p.numel() for p in self.params)
        for p in self.params:
            if p.dtype != torch.float64:
                raise ValueError("DataParallelTrainer expects float64 parameters (fp64 training path)")
        # flat parameter vector (reference state_dict order) and flat gradient buffer (+2 logging scalars);
        # every parameter / .grad becomes a view into them
        self.pflat = torch.empty(self.numel, dtype=torch.float64, device=p0.device)
        self.flat = torch.zeros(self.numel + 2, dtype=torch.float64, device=p0.device)
        off = 0
        for p in self.params:
            n = p.numel()
            self.pflat[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.pflat[off:off + n].view(p.shape)
            p.grad = self.flat[off:off + n].view(p.shape)
            off += n
        self._last = self.flat
        self.desc = None
        if fused and hasattr(model, 'fused_desc') and p0.is_cuda and len(self.params) == len(list(model.parameters())):
            from . import _lib
            desc = model.fused_desc()
            if _lib.model_param_count(desc) == self.numel:
                self.desc = desc
        if fused is True and self.desc is None:
            raise RuntimeError("fused training path requested but the model does not support it")
        kw = dict(optimizer_kwargs or {})
        if optimizer.lower() == 'lbfgs':
            # as the reference (solvers/solver_pt.py:154-155)
            raise NotImplementedError("LBFGS requires a closure; not supported by the current training loop.")
        opt_map = {'adam': torch.optim.Adam, 'adamw': torch.optim.AdamW, 'sgd': torch.optim.SGD,
                   'rmsprop': torch.optim.RMSprop}
        cls = opt_map.get(optimizer.lower(), torch.optim.Adam)
        if cls is torch.optim.Adam and p0.is_cuda and set(kw) <= {'betas', 'eps', 'weight_decay'}:
            self.optimizer = FlatAdam(self.params, self.pflat, self.flat, lr=lr, **kw)     # one launch per update
        else:
            if cls in (torch.optim.Adam, torch.optim.AdamW) and p0.is_cuda and 'fused' not in kw:
                kw['fused'] = True
            self.optimizer = cls(self.params, lr=lr, **kw)
        self.peer = None
        self.peer_fused = False              # the exchange runs inside the reduce kernel (qhea_model_dp_train_steps)
        self.fused_ok = True                 # ... and has not been found to stall on this placement of ranks (calibrate_exchange)
        self.dp_exchange_reason = "single rank: no exchange"
        if self.world > 1:
            self.broadcast_parameters()
            if not isinstance(self.optimizer, FlatAdam):
                self.dp_exchange_reason = "all_reduce: the peer exchange fuses the flat Adam update; this optimizer is torch's"
            elif not peer_exchange:
                self.dp_exchange_reason = "all_reduce: requested (peer_exchange=False / config dp_exchange)"
            else:
                self.peer, self.dp_exchange_reason = PeerExchange.create(dist, dist.get_rank(), self.world, self.numel + 2,
                                                                         p0.device, log=log)
                self.peer_fused = self.peer is not None and self.desc is not None
        self.device_sampled = self.train_sampling is not None and self.train_device_noise is not None
        # the loss the run trains on, chosen once: loss_and_grad, train_step and _steps go through this record
        self.train_loss = (self._jump_loss(log) if self.device_sampled else
                           self._sampled_loss(log) if self.train_sampling is not None else
                           self._exact_wide_loss(log) if self.train_noise_exact is not None else
                           self._exact_loss(log) if self.train_noise is not None else
                           self._exact_device_wide_loss(log) if self.train_device_noise_exact is not None else
                           self._exact_device_loss(log) if self.train_device_noise is not None else self._ideal_loss())

    def _ideal_loss(self):
        """the ideal loss (qhea_model_loss_grad / _train_step / _train_steps)"""
        from . import _lib
        return TrainLoss(lambda data, inv, grad, step, row0, ham_diag: _lib.model_loss_grad(*data, inv, grad, ham_diag=ham_diag),
                         lambda call, ham_diag: _lib.model_train_steps(*call, ham_diag=ham_diag), 'train_step', None)

    def _jump_loss(self, log):
        """train_device_noise with train_trajectories / train_jump_trajectories"""
        # the loss is the quantum-jump estimate under the device model (qhea_model_loss_grad_noisy_device at n = 7..9,
        # ..._noisy_device_lds at n = 10..12)
        key, nmax = self.sampling_key, 12 if self.sampling_key == 'train_jump_trajectories' else 9
        if self.desc is None or not isinstance(self.optimizer, FlatAdam):
            raise ValueError(f"train_device_noise with {key} needs the fused model-level path (a fp64 QuanONetPT "
                             "/ HEAQNNPT on a HIP device, Adam with betas / eps / weight_decay only)")
        from . import _lib
        n = self.desc.n_qubits
        if n <= 6:
            raise ValueError(f"train_device_noise with {key}: quantum-jump training takes n = 7..{nmax} (this model: "
                             f"n = {n}); for n <= 6 train_device_noise alone trains on the exact loss under the device model")
        if n > nmax:
            raise ValueError(f"train_device_noise with {key}: quantum-jump training takes n = 7..9 under this key (this "
                             f"model: n = {n}); train_jump_trajectories is the key that trains n = 7..12 on quantum-jump "
                             "trajectories under the DeviceNoise")
        try:
            hit = _lib.device_noise_singular_site(n, self.train_device_noise.params(n))
        except _lib.QheaError as e:
            raise ValueError(f"train_device_noise: {e}") from e
        if hit:
            raise ValueError(f"train_device_noise with {key}: relaxation site {hit[0]} on wire {hit[1]} has "
                             "gamma = 1, which the trajectory gradient cannot walk back")
        from .noise import check_jump_gradient_setting
        check_jump_gradient_setting(self.train_device_noise, n, f"train_device_noise with {key}")
        # the pair of calls for this qubit count: the wave-resident kernel at n = 7..9, the LDS-resident one at n = 10..12
        call_loss_grad, call_steps = _lib.device_sampled_grad_calls(n)

        def loss_grad(desc, branch, trunk, y, params, sampling, inv, grad, row0=0, ham_diag=None):
            return call_loss_grad(desc, branch, trunk, y, params, self.train_device_noise.params(n), sampling, inv, grad,
                                  row0=row0, ham_diag=ham_diag)

        def steps(*call, ham_diag=None):
            *head, sampling = call
            return call_steps(*head, self.train_device_noise.params(n), sampling, ham_diag=ham_diag)

        step_record = lambda step: _lib.SamplingParams(0, int(self.train_sampling.trajectories),
                                                       (int(self.train_sampling.seed) + int(step)) & ((1 << 64) - 1))
        if log is not None:
            log("device-noise training: the loss and 'loss_train' are the quantum-jump estimate of the MSE under the "
                f"DeviceNoise of train_device_noise, {self.train_sampling.trajectories} trajectories per row, stream seed "
                f"{self.train_sampling.seed} + step count")
        return _sampled_train_loss(loss_grad, steps, step_record)

    def _sampled_loss(self, log):
        """train_noise with train_sampling / train_trajectories"""
        # the loss is the sampled noisy one (qhea_model_loss_grad_noisy_wide / _lds): refuse here what the call would refuse
        key, nmax = self.sampling_key, 9 if self.sampling_key == 'train_sampling' else 12
        if self.desc is None or not isinstance(self.optimizer, FlatAdam):
            raise ValueError(f"{key} needs the fused model-level path (a fp64 QuanONetPT / HEAQNNPT on a HIP device, "
                             "Adam with betas / eps / weight_decay only)")
        if not 7 <= self.desc.n_qubits <= nmax:
            raise ValueError(f"{key}: sampled-trajectory training takes n = 7..{nmax} (this model: n = "
                             f"{self.desc.n_qubits}); for n <= 6 train_noise alone trains on the exact noisy loss")
        from . import _lib
        tn, sp = self.train_noise, self.train_sampling
        # train_noise's rates with train_sampling's trajectories and seed + step (mod 2^64)
        step_record = lambda step: _lib.NoiseParams(float(tn.p1), float(tn.p2), float(tn.readout), 0, int(sp.trajectories),
                                                    (int(sp.seed) + int(step)) & ((1 << 64) - 1))
        if log is not None:
            log(f"noise-aware training: the loss and 'loss_train' are the sampled noisy MSE under p1={self.train_noise.p1:g} "
                f"p2={self.train_noise.p2:g} readout={self.train_noise.readout:g}, {self.train_sampling.trajectories} "
                f"trajectories per row, stream seed {self.train_sampling.seed} + step count")
        return _sampled_train_loss(*_lib.sampled_grad_calls(self.desc.n_qubits), step_record)

    def _exact_loss(self, log):
        """train_noise alone"""
        # the loss is the exact noisy one (qhea_model_loss_grad_noisy_exact): refuse here what the call would refuse
        if self.desc is None or not isinstance(self.optimizer, FlatAdam):
            raise ValueError("train_noise needs the fused model-level path (a fp64 QuanONetPT / HEAQNNPT on a HIP device, "
                             "Adam with betas / eps / weight_decay only)")
        from . import _lib
        amp = _lib.model_exact_noisy_log10_amplification(self.desc, self.train_noise.params())
        if self.desc.n_qubits > 6 or not amp <= 12.0:
            raise ValueError(f"train_noise: noise-aware training takes n <= 6 and log10 amplification <= 12 (this model: "
                             f"n = {self.desc.n_qubits}, {amp:.2f}); see quanonet_amd.noise.amplification")
        if self.peer_fused:
            self.peer_fused = False
            self.dp_exchange_reason = ("peer exchange as a separate kernel: the noise-aware step has no reduce kernel with "
                                       "the exchange inside")
        if log is not None:
            log(f"noise-aware training: the loss and 'loss_train' are the exact noisy MSE under p1={self.train_noise.p1:g} "
                f"p2={self.train_noise.p2:g} readout={self.train_noise.readout:g} (log10 amplification {amp:.2f})")
        return _exact_train_loss(_lib.model_loss_grad_noisy_exact, _lib.model_train_steps_noisy_exact, self.train_noise.params)

    def _exact_wide_loss(self, log):
        """train_noise with train_noise_exact='wide': the exact noisy loss for every n it exists for"""
        # n <= 6 is the run that train_noise alone describes (qhea_model_loss_grad_noisy_exact); n = 7..9 trains on the same
        # loss with rho and O tiled through the workspace (qhea_model_loss_grad_noisy_exact_wide): refuse here what it would
        if self.desc is None or not isinstance(self.optimizer, FlatAdam):
            raise ValueError("train_noise_exact needs the fused model-level path (a fp64 QuanONetPT / HEAQNNPT on a HIP device, "
                             "Adam with betas / eps / weight_decay only)")
        n = self.desc.n_qubits
        if n <= 6:
            return self._exact_loss(log)
        from . import _lib
        amp = _lib.model_exact_noisy_log10_amplification(self.desc, self.train_noise.params())
        if n > 9 or not amp <= 12.0:
            raise ValueError(f"train_noise_exact='wide': the exact noisy loss takes n <= 9 and log10 amplification <= 12 (this "
                             f"model: n = {n}, {amp:.2f}); train_trajectories beside train_noise trains n = 7..12 on the "
                             "sampled loss; see quanonet_amd.noise.amplification")
        if self.peer_fused:
            # several ranks: loss_and_grad on the shard, then the exchange as a kernel of its own, the route of _exact_loss
            self.peer_fused = False
            self.dp_exchange_reason = ("peer exchange as a separate kernel: the noise-aware step has no reduce kernel with "
                                       "the exchange inside")
        base = _exact_train_loss(_lib.model_loss_grad_noisy_exact_wide, _lib.model_train_steps_noisy_exact_wide,
                                 self.train_noise.params)
        said = []

        def say(rows):
            # once, at the first call: only then is the batch known that the workspace is sized for
            if log is not None and not said:
                said.append(rows)
                log(f"noise-aware training: the loss and 'loss_train' are the exact noisy MSE under p1={self.train_noise.p1:g} "
                    f"p2={self.train_noise.p2:g} readout={self.train_noise.readout:g} (log10 amplification {amp:.2f}); rho and O "
                    f"are tiled through device memory, workspace "
                    f"{_lib.model_exact_noisy_wide_grad_workspace_bytes(self.desc, rows) / 2**20:.1f} MiB for steps of up to "
                    f"{rows} rows")

        def loss_grad(data, inv, grad, step, row0, ham_diag):
            say(int(data[3].numel()))                                    # data = (desc, branch, trunk, y, params)
            return base.loss_grad(data, inv, grad, step, row0, ham_diag)

        def steps(call, ham_diag):
            bounds = call[1]                                             # call = (desc, bounds, global_batches, ...)
            say(max((int(b) - int(a) for a, b in zip(bounds[:-1], bounds[1:])), default=0))
            return base.steps(call, ham_diag)
        return base._replace(loss_grad=loss_grad, steps=steps)

    def _exact_device_loss(self, log):
        """train_device_noise alone, rho walked back through inverses or replayed from stored states (train_noise_states)"""
        # the loss is the exact one under the device model (qhea_model_loss_grad_noisy_device_exact): the same refusals
        if self.desc is None or not isinstance(self.optimizer, FlatAdam):
            raise ValueError("train_device_noise needs the fused model-level path (a fp64 QuanONetPT / HEAQNNPT on a HIP "
                             "device, Adam with betas / eps / weight_decay only)")
        from . import _lib
        n = self.desc.n_qubits
        stored = self.noise_states == 'stored'
        try:
            rec = self.train_device_noise.params(n)
            amp = _lib.model_device_noisy_log10_amplification(self.desc, rec)
            # the library's own checks and bound
            refused = (_lib.model_device_noisy_stored_refused if stored else _lib.model_device_noisy_refused)(self.desc, rec)
            layer = _lib.model_device_noisy_log10_layer_amplification(self.desc, rec) if stored else None
        except _lib.QheaError as e:
            raise ValueError(f"train_device_noise: {e}") from e
        if refused and stored:
            raise ValueError(f"train_device_noise with train_noise_states='stored': the library refuses this model under "
                             f"this DeviceNoise (n = {n}, log10 amplification {amp:.2f}, of one layer {layer:.2f}): n <= 6 "
                             "and a layer amplification within the bound of include/quanonet_hea.h are needed; see "
                             "quanonet_amd.noise.device_layer_amplification")
        if refused:
            raise ValueError(f"train_device_noise: the library refuses this model under this DeviceNoise (n = {n}, log10 "
                             f"amplification {amp:.2f}): n <= 6 and a log10 amplification within the bound of "
                             "include/quanonet_hea.h are needed; see quanonet_amd.noise.device_amplification.  At "
                             "n = 7..9 train_trajectories beside train_device_noise trains on quantum-jump trajectories, "
                             "and train_jump_trajectories there does at n = 7..12; train_device_noise_exact='wide' beside "
                             "train_device_noise trains n = 7..9 on the exact loss")
        if self.peer_fused:
            self.peer_fused = False
            self.dp_exchange_reason = ("peer exchange as a separate kernel: the device-noise step has no reduce kernel "
                                       "with the exchange inside")
        if log is not None:
            log("device-noise training: the loss and 'loss_train' are the exact noisy MSE under the DeviceNoise of "
                f"train_device_noise (log10 amplification {amp:.2f})")
            if stored:
                per_row = _lib.model_device_noisy_stored_grad_workspace_bytes(self.desc, 1, snapshots_only=True)
                log(f"device-noise training: rho is replayed from stored states (train_noise_states='stored'; log10 "
                    f"amplification {amp:.2f} in total, {layer:.2f} for one layer, which is what the bound is asked of; "
                    f"{per_row} snapshot bytes per row)")
        calls = ((_lib.model_loss_grad_noisy_device_exact_stored, _lib.model_train_steps_noisy_device_exact_stored) if stored else
                 (_lib.model_loss_grad_noisy_device_exact, _lib.model_train_steps_noisy_device_exact))
        return _exact_train_loss(*calls, lambda: self.train_device_noise.params(n))

    def _exact_device_wide_loss(self, log):
        """train_device_noise with train_device_noise_exact='wide' or 'stored': the exact loss under the device model for every
        n it exists for"""
        # n <= 6 is the run that train_device_noise alone describes (train_noise_states honoured; 'stored' has set it); n = 7..9
        # trains on the same loss with rho and O tiled through the workspace ('wide': qhea_model_loss_grad_noisy_device_exact_wide,
        # the inverse walk; 'stored': ..._wide_stored, rho replayed from the states of the forward sweep): refuse here what
        # they would
        key = f"train_device_noise_exact={self.train_device_noise_exact!r}"
        if self.desc is None or not isinstance(self.optimizer, FlatAdam):
            raise ValueError("train_device_noise_exact needs the fused model-level path (a fp64 QuanONetPT / HEAQNNPT on a HIP "
                             "device, Adam with betas / eps / weight_decay only)")
        n = self.desc.n_qubits
        if n <= 6:
            return self._exact_device_loss(log)
        if n > 9:
            raise ValueError(f"{key}: the exact device-noisy loss takes n <= 9 (this model: n = {n}): "
                             "no density matrix of that size is carried; train_jump_trajectories beside train_device_noise "
                             "trains n = 7..12 on quantum-jump trajectories")
        if self.train_device_noise_exact == 'stored':
            return self._exact_device_wide_stored_loss(log)
        if self.noise_states == 'stored':
            raise ValueError("train_device_noise_exact='wide' with train_noise_states='stored' at n >= 7: the stored-state walk "
                             "does not exist on tiles under this value (its snapshots take units x rows x 16 x 4^n bytes); "
                             "'wide' trains n = 7..9 through the inverse walk, within its bound on device_amplification.  "
                             "train_device_noise_exact='stored' asks for the stored-state walk at every n = 2..9")
        from . import _lib
        try:
            rec = self.train_device_noise.params(n)
            amp = _lib.model_device_noisy_log10_amplification(self.desc, rec)
            refused = _lib.model_device_noisy_wide_refused(self.desc, rec)       # the library's own checks and bound
        except _lib.QheaError as e:
            raise ValueError(f"train_device_noise: {e}") from e
        if refused:
            raise ValueError(f"train_device_noise_exact='wide': the library refuses this model under this DeviceNoise (n = {n}, "
                             f"log10 A_dev = {amp:.2f}; the inverse walk's bound is 7 and a singular channel is inf); see "
                             "quanonet_amd.noise.device_amplification.  train_trajectories / train_jump_trajectories beside "
                             "train_device_noise train on quantum-jump trajectories whatever A_dev is")
        if self.peer_fused:
            # several ranks: loss_and_grad on the shard, then the exchange as a kernel of its own, the route of _exact_loss
            self.peer_fused = False
            self.dp_exchange_reason = ("peer exchange as a separate kernel: the device-noise step has no reduce kernel "
                                       "with the exchange inside")
        base = _exact_train_loss(_lib.model_loss_grad_noisy_device_exact_wide, _lib.model_train_steps_noisy_device_exact_wide,
                                 lambda: self.train_device_noise.params(n))
        said = []

        def say(rows):
            # once, at the first call: only then is the batch known that the workspace is sized for
            if log is not None and not said:
                said.append(rows)
                log("device-noise training: the loss and 'loss_train' are the exact device-noisy MSE under the DeviceNoise of "
                    f"train_device_noise (log10 A_dev {amp:.2f}); rho and O are tiled through device memory, workspace "
                    f"{_lib.model_device_noisy_wide_grad_workspace_bytes(self.desc, rows) / 2**20:.1f} MiB for steps of up to "
                    f"{rows} rows")

        def loss_grad(data, inv, grad, step, row0, ham_diag):
            say(int(data[3].numel()))                                    # data = (desc, branch, trunk, y, params)
            return base.loss_grad(data, inv, grad, step, row0, ham_diag)

        def steps(call, ham_diag):
            bounds = call[1]                                             # call = (desc, bounds, global_batches, ...)
            say(max((int(b) - int(a) for a, b in zip(bounds[:-1], bounds[1:])), default=0))
            return base.steps(call, ham_diag)
        return base._replace(loss_grad=loss_grad, steps=steps)

    def _exact_device_wide_stored_loss(self, log):
        """train_device_noise with train_device_noise_exact='stored' at n = 7..9: the loss of _exact_device_wide_loss with rho
        replayed from the states its forward sweep stored (qhea_model_loss_grad_noisy_device_exact_wide_stored)"""
        from . import _lib
        n = self.desc.n_qubits
        try:
            rec = self.train_device_noise.params(n)
            amp = _lib.model_device_noisy_log10_amplification(self.desc, rec)
            layer = _lib.model_device_noisy_log10_layer_amplification(self.desc, rec)
            refused = _lib.model_device_noisy_wide_stored_refused(self.desc, rec)    # the library's own checks and bound
        except _lib.QheaError as e:
            raise ValueError(f"train_device_noise: {e}") from e
        if refused:
            raise ValueError(f"train_device_noise_exact='stored': the library refuses this model under this DeviceNoise (n = {n}, "
                             f"log10 A_dev = {amp:.2f} in total, {layer:.2f} for one layer; the stored-state walk's bound is 7 "
                             "for one layer and a singular channel is inf); see quanonet_amd.noise.device_layer_amplification.  "
                             "train_trajectories / train_jump_trajectories beside train_device_noise train on quantum-jump "
                             "trajectories whatever A_dev is")
        if self.peer_fused:
            # several ranks: loss_and_grad on the shard, then the exchange as a kernel of its own, the route of _exact_loss
            self.peer_fused = False
            self.dp_exchange_reason = ("peer exchange as a separate kernel: the device-noise step has no reduce kernel "
                                       "with the exchange inside")
        base = _exact_train_loss(_lib.model_loss_grad_noisy_device_exact_wide_stored,
                                 _lib.model_train_steps_noisy_device_exact_wide_stored, lambda: self.train_device_noise.params(n))
        per_row = _lib.model_device_noisy_wide_stored_grad_workspace_bytes(self.desc, 1, snapshots_only=True)
        said = []

        def say(rows):
            # once, at the first call: only then is the batch known that the workspace is sized for
            if log is not None and not said:
                said.append(rows)
                log("device-noise training: the loss and 'loss_train' are the exact device-noisy MSE under the DeviceNoise of "
                    f"train_device_noise; rho is replayed from stored states (log10 A_dev {amp:.2f} in total, {layer:.2f} for "
                    f"one layer, which is what the bound is asked of; {per_row} snapshot bytes per row); rho, O and the "
                    "snapshots live in device memory, workspace "
                    f"{_lib.model_device_noisy_wide_stored_grad_workspace_bytes(self.desc, rows) / 2**20:.1f} MiB for steps of "
                    f"up to {rows} rows")

        def loss_grad(data, inv, grad, step, row0, ham_diag):
            say(int(data[3].numel()))                                    # data = (desc, branch, trunk, y, params)
            return base.loss_grad(data, inv, grad, step, row0, ham_diag)

        def steps(call, ham_diag):
            bounds = call[1]                                             # call = (desc, bounds, global_batches, ...)
            say(max((int(b) - int(a) for a, b in zip(bounds[:-1], bounds[1:])), default=0))
            return base.steps(call, ham_diag)
        return base._replace(loss_grad=loss_grad, steps=steps)

    def broadcast_parameters(self):
        self.dist.broadcast(self.pflat, src=0)

    def _forward(self, inputs):
        if isinstance(inputs, (tuple, list)):
            return self.model(*inputs)
        return self.model(inputs)

    def _ham_diag(self):
        q = getattr(self.model, 'quantum_layer', None)
        return q.ham_diag if (q is not None and getattr(q, 'use_full_ham', False)) else None

    @property
    def accepts_out(self):
        """Whether train_step can leave [gradients | sse | sum y^2] in a caller's buffer instead of self.flat (the fused
        model-level path with the flat Adam: nothing reads the parameters' .grad views there)."""
        return self.desc is not None and isinstance(self.optimizer, FlatAdam)

    def loss_and_grad(self, *batch, global_batch=None, out=None):
        """Fill self.flat (or `out`, see accepts_out) with this shard's [gradients | sse | sum y^2] (no collective, no
        update)."""
        *inputs, y = batch
        gb = float(global_batch if global_batch is not None else y.shape[0] * self.world)
        if self.desc is not None:
            data = (self.desc, *split_inputs(inputs), y.reshape(-1), self.pflat)
            grad = self.flat if out is None else out
            # (a sampled loss: the stream of the NEXT update, global rows from 0)
            self.train_loss.loss_grad(data, 1.0 / gb, grad, self.optimizer.t + 1, 0, self._ham_diag())
        else:
            self.flat.zero_()
            pred = self._forward(inputs)
            resid = pred - y.reshape(pred.shape)
            sse = (resid * resid).sum()
            (sse / gb).backward()
            with torch.no_grad():
                self.flat[self.numel] = sse
                self.flat[self.numel + 1] = (y * y).sum()
        return self.flat

    def train_step(self, *batch, global_batch=None, out=None, row0=0):
        """batch = (branch, trunk, y) or (x, y): this rank's shard.  Returns the flat buffer (device): self.flat, or
        `out` -- a caller's [numel + 2] fp64 buffer, honoured where accepts_out says so (PTSolver hands in one row per
        step of an epoch, so that the two logging scalars of every step stay on the device without a copy).
        row0 (train_sampling / train_trajectories only): the global index of the batch's first row, which keys its random
        streams -- a step of train_steps has its bounds[i] there."""
        if out is not None and not self.accepts_out:
            out = None
        flat = self._last = self.flat if out is None else out
        if self.world == 1 and self.desc is not None and isinstance(self.optimizer, FlatAdam):
            # single device: loss, gradients and the Adam update in three launches (qhea_model_train_step)
            from . import _lib
            *inputs, y = batch
            gb = float(global_batch if global_batch is not None else y.shape[0])
            opt = self.optimizer
            opt.t += 1
            if self.train_loss.single == 'loss_grad+adam':
                self.train_loss.loss_grad((self.desc, *split_inputs(inputs), y.reshape(-1), self.pflat), 1.0 / gb, flat, opt.t,
                                          int(row0), self._ham_diag())
                _lib.adam_step(self.pflat, flat, opt.exp_avg, opt.exp_avg_sq, opt.t, *opt.hparams())
            elif self.train_loss.single == 'steps':         # (the exact noisy losses have the steps entry only: one step of it)
                self._steps(inputs, y, [0, y.shape[0]], [gb], flat.view(1, -1), opt.t)
            else:
                _lib.model_train_step(self.desc, *split_inputs(inputs), y.reshape(-1), self.pflat, 1.0 / gb, flat, opt.exp_avg,
                                      opt.exp_avg_sq, opt.t, *opt.hparams(), ham_diag=self._ham_diag())
            return flat
        gb_all = float(global_batch if global_batch is not None else batch[-1].shape[0] * self.world)
        if self.peer_fused and gb_all >= self.world and batch[-1].shape[0] > 0:
            # the sum over the ranks inside this step's reduce kernel (qhea_model_dp_train_steps, one step).  Every rank
            # must take the same path: the choice rests on the GLOBAL batch (contiguous near-even shards, shard_slice,
            # are all non-empty when it is at least the world size)
            from . import _lib
            *inputs, y = batch
            gb = gb_all
            try:
                self._dp_steps(inputs, y, [0, y.shape[0]], [gb], flat.view(1, -1))
                return flat
            except _lib.Unsupported:
                self.peer_fused = False                 # reduce grid not resident at once: separate exchange kernel from now on
        self.loss_and_grad(*batch, global_batch=global_batch, out=out)
        if self.peer is not None:
            # sum over the ranks' peer-mapped buffers + Adam in ONE launch (csrc/hea_dp.hip)
            self.peer.allreduce_adam(flat, self.pflat, self.optimizer)
            return flat
        if self.world > 1:
            self.dist.all_reduce(flat)                 # SUM; one latency-bound message (19 KB at Q5)
        if out is not None:                            # FlatAdam reads its gradient from self.flat
            self.flat.copy_(out)
        self.optimizer.step()
        return flat

    def _steps(self, inputs, y, bounds, global_batches, rows, first_step):
        """single device: the steps entry, ideal (qhea_model_train_steps), under train_noise (..._noisy_exact; with
        train_sampling / train_trajectories ..._noisy_wide or ..._noisy_lds) or under train_device_noise
        (..._noisy_device_exact, with train_noise_states='stored' ..._noisy_device_exact_stored)"""
        opt = self.optimizer
        call = (self.desc, bounds, global_batches, *split_inputs(inputs), y.reshape(-1), self.pflat, rows, opt.exp_avg,
                opt.exp_avg_sq, first_step, *opt.hparams())
        self.train_loss.steps(call, self._ham_diag())

    def _dp_steps(self, inputs, y, bounds, global_batches, rows):
        from . import _lib
        opt, px = self.optimizer, self.peer
        n_steps = len(bounds) - 1
        _lib.model_dp_train_steps(self.desc, bounds, global_batches, *split_inputs(inputs), y.reshape(-1), self.pflat, rows,
                                  opt.exp_avg, opt.exp_avg_sq, opt.t + 1, *opt.hparams(), px.rank, px.world, px.bufs,
                                  px.n, px.seq + 1, timeout_ms=px.timeout_ms, ham_diag=self._ham_diag())
        opt.t += n_steps
        px.seq += n_steps

    def calibrate_exchange(self, *batch, global_batch=None, steps=30):
        """
        Several ranks, peer buffers mapped: time this very step through both forms of the peer exchange -- inside the
        reduce kernel (two launches per step) and as a separate one-workgroup kernel (four) -- and keep the faster one.
        Which one wins depends on where the ranks run: the reduce kernel's waiting blocks hold compute units, which costs
        nothing when every rank has a GPU of its own and a lot when ranks share one (a rehearsal).  Collective; parameters,
        Adam state and step count are restored afterwards, so a run is the same with or without the calibration.  Returns
        (ms per step fused, ms per step separate) or None when there is nothing to choose.
        """
        if not self.peer_fused or self.world < 2:
            return None
        import time
        gb = float(global_batch if global_batch is not None else batch[-1].shape[0] * self.world)
        if gb < self.world or batch[-1].shape[0] == 0:
            return None
        from . import _lib
        opt = self.optimizer
        keep = (self.pflat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.t)
        dev = self.pflat.device

        def restore():
            self.pflat.copy_(keep[0]); opt.exp_avg.copy_(keep[1]); opt.exp_avg_sq.copy_(keep[2]); opt.t = keep[3]

        def timed(fused):
            self.peer_fused = fused
            for _ in range(2):                                   # the first pass warms up
                self.dist.barrier(); torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(steps):
                    self.train_step(*batch, global_batch=global_batch)
                torch.cuda.synchronize(dev)
                dt = time.perf_counter() - t0
            bad = 0.0
            try:
                self.peer.check_status()
            except _lib.QheaError:
                bad = 1.0
            t = torch.tensor([dt, bad], dtype=torch.float64, device=dev)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            return 1e3 * float(t[0].item()) / steps, bool(t[1].item() > 0.5)
        # The trial inside the reduce kernel runs with a short bound: where ranks SHARE a GPU its waiting blocks can keep a
        # peer's kernels off the compute units for good (seen with three ranks on one device).  A failed trial has poisoned
        # the buffers (a timeout is fatal by design): they are re-created and the separate kernel is kept.
        long_timeout, self.peer.timeout_ms = self.peer.timeout_ms, 250.0
        t_fused, failed = timed(True)
        self.peer.timeout_ms = long_timeout
        if failed:
            restore()
            torch.cuda.synchronize(dev)
            self.peer.close()
            self.peer, why = PeerExchange.create(self.dist, self.dist.get_rank(), self.world, self.numel + 2, dev)
            self.peer_fused = False
            self.fused_ok = False
            self.dp_exchange_reason = (why + "; calibrated on this step: the exchange inside the reduce kernel did not complete "
                                       "within 250 ms (ranks sharing a GPU?) -> separate kernel, buffers re-created")
            return None
        p_fused = self.pflat.clone()
        restore()
        t_sep, failed = timed(False)
        p_sep = self.pflat.clone()
        restore()
        if failed:
            raise _lib.QheaError("data-parallel exchange failed during calibration")
        # Both trials ran the same steps from the same state, and both add the ranks' numbers in rank order: the parameters
        # they end on must be BITWISE the same, on every rank.  Checked here because this is the first place the exchange
        # meets the run's real placement of ranks (separate GPUs, the link between them): if the two forms disagree or
        # the replicas differ, neither is trusted and every rank keeps the collective library's all-reduce.
        if not self._agree_bitwise(p_fused, p_sep):
            torch.cuda.synchronize(dev)
            self.peer.close()
            self.peer = None
            self.peer_fused = False
            self.fused_ok = False
            self.dp_exchange_reason += ("; calibrated on this step: the two forms of the peer exchange did NOT end on bitwise "
                                        "identical parameters on every rank -> all_reduce (collective library) + Adam launch")
            return None
        # (the same numbers on every rank: one decision.  Within 3 % the form inside the reduce kernel is kept: it lets an epoch's
        # inner loop be ONE host call, which this per-step timing does not credit it with)
        self.peer_fused = t_fused <= 1.03 * t_sep
        self.dp_exchange_reason += (f"; calibrated on this step: {t_fused:.4f} ms inside the reduce kernel, {t_sep:.4f} ms "
                                    f"as a separate kernel, parameters bitwise identical through both and on every rank -> "
                                    + ("inside the reduce kernel" if self.peer_fused else "separate kernel"))
        return t_fused, t_sep

    def _agree_bitwise(self, a, b):
        """Collective: True on every rank iff a == b bitwise on every rank AND every rank holds rank 0's a and b."""
        ref = torch.stack([a, b])
        self.dist.broadcast(ref, src=0)
        wrong = torch.tensor([0.0 if (torch.equal(a, b) and torch.equal(ref[0], a) and torch.equal(ref[1], b)) else 1.0],
                             dtype=torch.float64, device=a.device)
        self.dist.all_reduce(wrong, op=self.dist.ReduceOp.MAX)
        return wrong.item() < 0.5

    @property
    def epoch_call(self):
        """Whether train_steps can issue a run of steps from one host call: the fused single-device path, or the
        data-parallel path with the exchange inside the reduce kernel."""
        return self.accepts_out and (self.world == 1 or self.peer_fused)

    def train_steps(self, inputs, y, bounds, global_batches, rows):
        """
        The steps of a whole epoch from ONE host call -- step i on rows bounds[i]:bounds[i+1] of the contiguous `inputs` /
        `y` (this rank's shards), its [gradients | sse | sum y^2] (summed over the ranks) left in rows[i].  One device:
        qhea_model_train_steps; several: qhea_model_dp_train_steps, the sum over the ranks inside each step's reduce kernel
        (raises _lib.Unsupported, nothing launched, if a shard is empty).  Bitwise the result of calling
        train_step(..., out=rows[i]) in a loop, without the interpreter between launches.
        """
        assert self.epoch_call
        n_steps = len(bounds) - 1
        if self.world > 1:
            self._dp_steps(inputs, y, bounds, global_batches, rows)
        else:
            self._steps(inputs, y, bounds, global_batches, rows, self.optimizer.t + 1)
            self.optimizer.t += n_steps
        self._last = rows[n_steps - 1]
        return rows

    def loss_scalars(self):
        """(sse, sum y^2) of the last global batch -- forces a device sync; call per epoch, not per step."""
        v = self._last[self.numel:].tolist()        # the buffer the last step left its results in (self.flat or `out`)
        return v[0], v[1]

    def check_status(self):
        """Raise if a backward kernel reported a hand-off overrun since the last check (qhea_check_status; that call's
        gradients were NaN-poisoned and its Adam update skipped).  Synchronises: call where the host waits anyway."""
        if not self.pflat.is_cuda:
            return
        from . import _lib
        err = None
        try:
            _lib.check_status(self.pflat.device)
            if self.peer is not None:
                self.peer.check_status()
        except _lib.QheaError as e:
            err = e
        if self.world > 1:
            # the ranks agree on the outcome BEFORE anybody acts on it (rank 0 saving a checkpoint): a failure
            # on any rank raises on every rank
            t = torch.tensor([0.0 if err is None else 1.0], dtype=torch.float64, device=self.pflat.device)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            if err is None and t.item() > 0.5:
                err = _lib.QheaError("a peer rank reported a failed step (pipeline overrun or exchange timeout): "
                                     "the replicas are no longer in step")
        if err is not None:
            raise err


class PTSolver:
    """
    Mirror of the reference PTSolver (solvers/solver_pt.py:21-329).  ``config`` uses the reference's
    keys (model_type, operator, num_qubits, net_size, scale_coeff, if_trainable_freq, ham_bound,
    ham_diag, learning_rate, batch_size, num_epochs, optimizer, lr_scheduler, if_save, prefix, seed).
    ``data_dict`` has the DataManager output keys (data_utils/data_manager.py:74-106):
    train_branch_input/train_trunk_input/train_output/test_* (QuanONet) or train_input/... (HEAQNN).
    """

    def __init__(self, config, data_dict, device=None, dist=None, rank=0, world_size=1, log=print, model=None):
        self.config = config
        self.data_dict = data_dict
        self.model_type = config['model_type']
        self.dist, self.rank, self.world = dist, rank, world_size
        self.log = log if rank == 0 else (lambda *a, **k: None)
        self.device = device if device is not None else torch.device('cuda')
        # `model` is a seam for the host-logic tests (a module whose quantum layer is the oracle test double runs
        # this very loop on the CPU); the solver never builds anything but the HIP modules itself
        if self.device.type != 'cuda' and model is None:
            raise RuntimeError("PTSolver runs on a HIP device only (no CPU fallback)")
        self.out_dir = run_dir(config)
        self.model = (model if model is not None else self._create_model()).to(self.device)
        self.trainer = DataParallelTrainer(self.model, lr=config['learning_rate'], world_size=world_size,
                                           dist=dist, optimizer=config.get('optimizer', 'adam'),
                                           optimizer_kwargs=config.get('optimizer_kwargs', {}),
                                           peer_exchange=str(config.get('dp_exchange', 'peer')).lower() == 'peer',
                                           log=self.log, train_noise=config.get('train_noise'),
                                           train_device_noise=config.get('train_device_noise'),
                                           train_sampling=config.get('train_sampling'),
                                           train_trajectories=config.get('train_trajectories'),
                                           train_jump_trajectories=config.get('train_jump_trajectories'),
                                           train_noise_states=config.get('train_noise_states'),
                                           train_noise_exact=config.get('train_noise_exact'),
                                           train_device_noise_exact=config.get('train_device_noise_exact'))
        self.lr_scheduler = self._build_scheduler()
        self.best_loss = float('inf')
        self.best_model_path = None
        self._setup_data()

    # ---- model / data -------------------------------------------------------------------------
    def _create_model(self):
        from .models import QuanONetPT, HEAQNNPT
        c = self.config
        ham_bound, net_size = model_setting(c, 'ham_bound'), model_setting(c, 'net_size')
        if_tf, scale = model_setting(c, 'if_trainable_freq'), model_setting(c, 'scale_coeff')
        n = int(c['num_qubits'])
        # --ham_diag strictly overrides --ham_pauli (utils/common.py:84)
        ham_pauli = 'Z' if c.get('ham_diag') is not None else (c.get('ham_pauli') or 'Z')
        if self.model_type == 'QuanONet':
            return QuanONetPT(n, self.data_dict['train_branch_input'].shape[1],
                              self.data_dict['train_trunk_input'].shape[1], net_size, scale_coeff=scale,
                              if_trainable_freq=if_tf, ham_bound=ham_bound, ham_diag=c.get('ham_diag'),
                              ham_pauli=ham_pauli)
        if self.model_type == 'HEAQNN':
            return HEAQNNPT(n, self.data_dict['train_input'].shape[1], net_size, scale_coeff=scale,
                            if_trainable_freq=if_tf, ham_bound=ham_bound, ham_diag=c.get('ham_diag'),
                            ham_pauli=ham_pauli)
        raise ValueError(f"PTSolver does not support model_type='{self.model_type}'")

    def _dev(self, a):
        return torch.as_tensor(np.asarray(a), dtype=torch.float64).to(self.device)

    def _setup_data(self):
        d = self.data_dict
        if self.model_type == 'HEAQNN':
            self.train_input = (self._dev(d['train_input']),)
            self.test_input = (self._dev(d['test_input']),)
        else:
            self.train_input = (self._dev(d['train_branch_input']), self._dev(d['train_trunk_input']))
            self.test_input = (self._dev(d['test_branch_input']), self._dev(d['test_trunk_input']))
        self.train_output = self._dev(d['train_output']).reshape(len(d['train_output']), -1)
        self.test_output = np.asarray(d['test_output'], dtype=np.float64).reshape(len(d['test_output']), -1)

    def _build_scheduler(self):
        name = str(self.config.get('lr_scheduler', 'none')).lower()
        kw = self.config.get('lr_scheduler_kwargs', {})
        opt = self.trainer.optimizer
        if name == 'cosine':
            return torch.optim.lr_scheduler.CosineAnnealingLR(
                opt, T_max=kw.get('T_max', self.config.get('num_epochs', 1000)), eta_min=kw.get('eta_min', 0.0))
        if name == 'step':
            return torch.optim.lr_scheduler.StepLR(opt, step_size=kw.get('step_size', 100), gamma=kw.get('gamma', 0.5))
        if name == 'exponential':
            return torch.optim.lr_scheduler.ExponentialLR(opt, gamma=kw.get('gamma', 0.99))
        return None

    # ---- training (solver_pt.py:191-277) ------------------------------------------------------------
    def _save(self, path, flat=None):
        """state_dict as .pt + .npz.  `flat`: a (host) snapshot of the trainer's flat parameter vector to save INSTEAD of the
        live parameters -- the epoch loop has already queued the next epoch when it decides about the checkpoint (train())."""
        sd = self.model.state_dict()
        if flat is not None:
            sd = dict(sd)
            own = {id(p): i for i, p in enumerate(self.trainer.params)}
            offs = np.cumsum([0] + [p.numel() for p in self.trainer.params])
            for k, p in self.model.named_parameters():
                i = own.get(id(p))
                if i is not None and k in sd:
                    sd[k] = flat[offs[i]:offs[i + 1]].view(p.shape).to(sd[k].dtype)
        torch.save(sd, path)
        np.savez(path.replace('.pt', '.npz'), **{k: v.detach().cpu().numpy() for k, v in sd.items()})

    def _stage_epoch(self, n, bs, nb):
        """
        One epoch's batch order and this rank's rows of it, gathered ONCE (three gathers per epoch instead of three per
        step): step i of the reference takes idx[i*bs:(i+1)*bs] (solver_pt.py:226-228), this rank its contiguous shard
        of that.  Returns (order, row bounds per step, gathered inputs, gathered targets).
        """
        idx_dev = self._epoch_permutation(n)
        bounds, pieces = [0], []
        for i in range(nb):
            gb_i = min(bs, n - i * bs)
            lo, hi = shard_slice(gb_i, self.rank, self.world)
            pieces.append((i * bs + lo, i * bs + hi))
            bounds.append(bounds[-1] + hi - lo)
        if self.world == 1:
            sel_all = idx_dev
        else:
            sel_all = torch.cat([idx_dev[a:b] for a, b in pieces]) if bounds[-1] else idx_dev[:0]
        return idx_dev, bounds, [t[sel_all] for t in self.train_input], self.train_output[sel_all]

    def _epoch_permutation(self, n):
        """
        ``np.random.permutation(n)`` from NumPy's global generator, as the reference draws it (solver_pt.py:220), so a
        launcher that seeds like the reference's (``set_random_seed``) reproduces its batch order.  With several
        ranks ONLY rank 0 draws and the order is broadcast: every rank then slices the same global batch whatever
        its own generator state is (separately launched ranks are not seeded alike by anything).
        """
        if self.world > 1:
            idx = torch.empty(n, dtype=torch.int64, device=self.device)
            if self.rank == 0:
                idx.copy_(torch.as_tensor(np.random.permutation(n)))
            self.dist.broadcast(idx, src=0)
            return idx
        return torch.as_tensor(np.random.permutation(n), device=self.device)

    def _record_epoch(self, epoch, history, tl, gbs, snap, want_save, log, tag=''):
        """
        One epoch's loss accounting (solver_pt.py:243-262): its mean batch MSE into history['loss_train'], the best-by-train-loss
        checkpoint from `snap` (the host copy of the parameters at the epoch's end) and a log line every 10 epochs.  tl: the
        epoch's [sse, sum y^2] per step.  Returns the steps' MSE.
        """
        avg_loss, sse, sum_y2, step_mse = epoch_sums(tl, gbs)
        history['loss_train'].append(avg_loss)
        if avg_loss < self.best_loss:
            self.best_loss = avg_loss
            if want_save:
                self._save(self.best_model_path, flat=snap)
        if epoch % 10 == 0:
            avg_rel = np.sqrt(sse) / (np.sqrt(sum_y2) + 1e-8)
            log(f"{tag}Epoch {epoch} | MSE: {avg_loss:.6e} | Rel_L2: {avg_rel:.4%}")
        return step_mse

    def is_completed(self):
        """Whether this run's directory already holds a metric.json -- the reference's "experiment already completed" test
        (utils/logger.py:182-185), on which its train() ends the process (solvers/solver_pt.py:192-194)."""
        return os.path.exists(os.path.join(self.out_dir, 'metric.json'))

    def train(self):
        if self.config.get('skip_completed', False) and self.is_completed():
            # the reference calls sys.exit(0) here; a library returns instead (the launcher decides what to do with None)
            self.log("Experiment already completed (metric.json exists): training skipped.")
            return None
        n = self.train_output.shape[0]
        bs = min(int(self.config.get('batch_size', 100)), n)
        epochs = int(self.config['num_epochs'])
        nb, gbs, _ = batch_plan(n, bs)                          # (the row bounds are this rank's: _stage_epoch)
        history = {'loss_train': [], 'loss_test': []}
        trace = bool(self.config.get('trace_steps', False))     # parity tests: per-step MSE and the epoch orders
        if trace:
            history['loss_steps'], history['indices'] = [], []
        os.makedirs(self.out_dir, exist_ok=True)
        self.best_model_path = os.path.join(self.out_dir, 'best_model.pt')
        first = self._stage_epoch(n, bs, nb) if epochs > 0 else None
        if first is not None and self.world > 1 and self.config.get('dp_calibrate', True):
            # both forms of the peer exchange timed on the first batch, the faster one kept (state restored afterwards)
            _, b0, in0, out0 = first
            r = self.trainer.calibrate_exchange(*[t[b0[0]:b0[1]] for t in in0], out0[b0[0]:b0[1]], global_batch=gbs[0])
            if r is not None:
                self.log("data-parallel exchange: " + self.trainer.dp_exchange_reason)
        want_save = self.config.get('if_save', True) and self.rank == 0
        nm = self.trainer.numel

        def issue(staged):
            """queue one epoch's steps; returns the device rows of its [sse | sum y^2] and its order"""
            self.model.train()
            idx_dev, bounds, ep_inputs, ep_output = staged
            # (sse, sum y^2) of every global batch stay on the device until the epoch ends.  On the fused path every step
            # leaves its [gradients | sse | sum y^2] in a row of its own (no copy kernel per step; nb x 19 KB at Q5)
            rows = (torch.zeros(nb, nm + 2, dtype=torch.float64, device=self.device) if self.trainer.accepts_out
                    else None)
            tails = rows[:, nm:] if rows is not None else torch.zeros(nb, 2, dtype=torch.float64, device=self.device)
            # the whole epoch's inner loop from one host call (no interpreter between the launches; config['epoch_call'] =
            # False keeps one host call per step).  Several ranks: every rank must take the same path, so the choice rests on
            # what all of them know -- no global batch smaller than the world size (an empty shard somewhere)
            one_call = (rows is not None and self.trainer.epoch_call and self.config.get('epoch_call', True) and
                        gbs[-1] >= self.world)
            if one_call:
                self.trainer.train_steps(ep_inputs, ep_output, bounds, gbs, rows)
            else:
                for i in range(nb):
                    a, b = bounds[i], bounds[i + 1]
                    flat = self.trainer.train_step(*[t[a:b] for t in ep_inputs], ep_output[a:b], global_batch=gbs[i],
                                                   out=None if rows is None else rows[i], row0=a)
                    if rows is None:
                        tails[i].copy_(flat[nm:])
            return tails, idx_dev

        def snapshot(idx_dev):
            return (self.trainer.pflat.detach().to('cpu', copy=True) if want_save else None,
                    idx_dev.cpu().numpy() if trace else None)

        def record(epoch, tl, snap):
            step_mse = self._record_epoch(epoch, history, tl, gbs, snap[0], want_save, self.log)
            if trace:
                history['loss_steps'].extend(step_mse)
                history['indices'].append(snap[1])

        run_epochs(epochs, first, lambda: self._stage_epoch(n, bs, nb), issue, self.trainer.check_status, snapshot,
                   [self.lr_scheduler] if self.lr_scheduler is not None else [], record)
        if self.config.get('if_save', True) and self.rank == 0:
            self._save(os.path.join(self.out_dir, 'final.pt'))                 # logger.py:174-177 + solver_pt.py:266-272: final.pt / final.npz
        return history

    # ---- evaluation (solver_pt.py:279-329, utils/metrics.py:6-29) -----------------------------------------
    def predict(self, inputs, batch_size=None):
        bs = int(batch_size or self.config.get('batch_size', 100))
        n = inputs[0].shape[0]
        outs = []
        self.model.eval()
        tr = self.trainer
        with torch.no_grad():
            if tr.desc is not None and n > 0:
                # all chunks from one host call: the layer records are prepared once for the whole set (the parameters
                # do not change during an evaluation)
                from . import _lib
                o = _lib.model_forward_chunks(tr.desc, *split_inputs([t.contiguous() for t in inputs]), tr.pflat, bs,
                                              ham_diag=tr._ham_diag())
                return o.unsqueeze(-1)
            for s in range(0, n, bs):
                chunk = [t[s:s + bs] for t in inputs]
                outs.append(self.model(*chunk))
        if not outs:                                            # an empty shard (fewer test rows than ranks)
            return torch.empty((0, 1), dtype=torch.float64, device=inputs[0].device)
        return torch.cat(outs, dim=0)

    def _load_best(self):
        """the best-by-train-loss checkpoint into the model, where train() wrote one"""
        if self.best_model_path and os.path.exists(self.best_model_path):
            sd = torch.load(self.best_model_path, map_location=self.device, weights_only=True)
            self.model.load_state_dict(sd)

    def evaluate(self, history=None):
        # rank 0 alone wrote best_model.pt (train()) and alone reads it back; the other ranks receive the weights by
        # broadcast (parameters are views into the trainer's flat vector), so no rank can read a half-written file
        # or, on node-local storage, silently evaluate different weights
        if self.rank == 0:
            self._load_best()
        if self.world > 1:
            self.trainer.broadcast_parameters()
        # every rank evaluates its contiguous slice of the test set (10-100x a training batch: SURVEY.md 8(f)-2) in
        # chunks of 16384 rows (Q5: 87 M evaluations/s against 27 M at 1024 rows per call, profiles/r02_batch_sweep.txt);
        # the metrics are reduced from four sums and one maximum
        n_test = self.test_input[0].shape[0]
        lo, hi = shard_slice(n_test, self.rank, self.world)
        y_pred = self.predict([t[lo:hi] for t in self.test_input], batch_size=self.config.get('eval_batch_size', 16384))
        y_true = torch.as_tensor(np.asarray(self.test_output)[lo:hi], dtype=torch.float64).to(y_pred.device)
        metrics = regression_metrics(y_pred, y_true, self.dist, self.world)
        if self.rank == 0:
            os.makedirs(self.out_dir, exist_ok=True)
            with open(os.path.join(self.out_dir, 'metric.json'), 'w') as f:
                json.dump({'metrics': metrics, 'history': history}, f, default=lambda o: o.tolist())
        self.log(f"Test Relative L2 Error: {metrics['rel_l2']:.6f}")
        return metrics

    def evaluate_noisy(self, noise, out_name=None, exact=False, sampling=None):
        """
        The test set of `evaluate` predicted under `noise` (a quanonet_amd.noise.NoiseModel) from the best checkpoint:
        regression_metrics plus 'mean_stderr' (the rows' mean standard error) and 'noise' (the settings).  Writes
        out_dir/out_name when out_name is given and never touches metric.json (the run's "completed" marker).  Single rank.
        exact=True: the metrics of the exact expectation under the noise channels (exact_noisy_predict; no sampling error,
        noise.shots / trajectories / seed ignored), with 'exact': True and 'mean_shot_std' (the rows' mean one-shot standard
        deviation) in place of 'mean_stderr'.  A quanonet_amd.noise.DeviceNoise (per-wire rates, T1 / T2, the ring's idle
        decay) is evaluated with exact=True, or sampled with sampling= (a quanonet_amd.noise.Sampling: quantum-jump trajectories,
        device_noisy_predict; 'mean_stderr', and 'sampling' beside 'noise').  sampling belongs to a DeviceNoise without exact.
        exact='wide': the same result through wide_exact_noisy_predict, which also serves n = 7..9 (the density matrix tiled
        through device memory; a NoiseModel only at those sizes); exact=True keeps refusing n >= 7.
        exact='device': a DeviceNoise through device_exact_noisy_predict, n = 2..9 (its channel sites on the same tiles); the same
        metric keys as exact=True.
        """
        from .noise import (DeviceNoise, _TRAJECTORY_WHY, _uniform_only, device_exact_noisy_predict, device_noisy_predict,
                            exact_noisy_predict, noisy_predict, wide_exact_noisy_predict)
        if self.world > 1:
            raise RuntimeError("evaluate_noisy runs on one rank (world_size == 1)")
        if isinstance(exact, str) and exact not in ('wide', 'device'):
            raise ValueError(f"evaluate_noisy: exact={exact!r}; exact is False, True (n <= 6), 'wide' (n <= 9) or 'device' "
                             "(a DeviceNoise, n <= 9)")
        if exact == 'device' and not isinstance(noise, DeviceNoise):
            raise ValueError(f"evaluate_noisy: exact='device' evaluates a DeviceNoise (got {type(noise).__name__}); a NoiseModel "
                             "goes to exact='wide', or through DeviceNoise.uniform")
        if sampling is not None and (exact or not isinstance(noise, DeviceNoise)):
            raise ValueError("evaluate_noisy: sampling= is the estimator of a DeviceNoise's trajectories; exact=True draws "
                             "nothing and a NoiseModel carries its own shots, trajectories and seed")
        if not exact and sampling is None:
            _uniform_only(noise, 'evaluate_noisy(exact=False)', _TRAJECTORY_WHY)
        self._load_best()
        chunk_rows = self.config.get('eval_batch_size', 16384)
        if sampling is not None:
            y_pred, stderr = device_noisy_predict(self.model, self.test_input, noise, sampling, chunk_rows=chunk_rows)
        else:
            predict = wide_exact_noisy_predict if exact == 'wide' else device_exact_noisy_predict if exact == 'device' else \
                exact_noisy_predict if exact else noisy_predict
            y_pred, stderr = predict(self.model, self.test_input, noise, chunk_rows=chunk_rows)
        y_true = torch.as_tensor(np.asarray(self.test_output), dtype=torch.float64).to(y_pred.device)
        metrics = regression_metrics(y_pred, y_true)
        spread = 'mean_shot_std' if exact else 'mean_stderr'
        metrics[spread] = float(stderr.mean().item()) if stderr.numel() else 0.0
        metrics['noise'] = noise.asdict()
        if sampling is not None:
            metrics['sampling'] = sampling.asdict()
        if exact:
            metrics['exact'] = True
        if out_name:
            os.makedirs(self.out_dir, exist_ok=True)
            with open(os.path.join(self.out_dir, out_name), 'w') as f:
                json.dump(metrics, f)
        self.log(f"Noisy test Relative L2 Error: {metrics['rel_l2']:.6f} ({spread.replace('_', ' ')} {metrics[spread]:.3g})")
        return metrics
