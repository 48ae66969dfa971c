"""
Model-ensemble training: the seeds of one configuration trained side by side on one device, every step of all R members as
ONE launch per kernel (qhea_model_ensemble_train_steps: member = the grid's second dimension).  The reference starts the
seeds of a sweep cell as concurrent processes (scripts/reproduce_benchmarks2.sh, its `for SEED` loop); at the paper's batch
of 100 one model leaves most of the device idle, R models in one grid fill it.  Shapes with n <= 5 (ZYZ kernels) and n >= 10
(workgroup-resident kernels) take the one-grid path; n = 6..9 train as R consecutive single-model calls.

Member m is exactly the PTSolver run its config describes when launched after ``set_random_seed(seed_m)``: its model is
built right after ``torch.manual_seed(seed_m)``, its batch order is drawn per epoch from ``np.random.RandomState(seed_m)``
(the sequence NumPy's global generator gives after ``np.random.seed(seed_m)``), and it keeps its own best / final
checkpoints in the directory ``PTSolver(config_m)`` uses.
"""
import os

import numpy as np
import torch

from .solver import PTSolver, batch_plan, model_setting, run_epochs, split_inputs

# keys in which the members of one ensemble may differ (scale_coeff too, for trainable-frequency models: there it only sets
# the initial frequency weights, the descriptor the kernels see is shared)
MEMBER_KEYS = ('seed', 'run_id', 'prefix')


def check_supported(configs, who='EnsembleSolver'):
    """Raise ValueError for settings no one-launch-per-step training supports (the checks every member must pass alone)."""
    configs = list(configs)
    if not configs:
        raise ValueError(f"{who} needs at least one config")
    for c in configs:
        if int(c.get('world_size', 1)) > 1:
            raise ValueError(f"{who} runs on one device: world_size > 1 is not supported")
        dp = sorted(k for k in c if k.startswith('dp_'))
        if dp:
            raise ValueError(f"{who} has no data-parallel step: remove {dp}")
        if str(c.get('optimizer', 'adam')).lower() != 'adam':
            raise ValueError(f"{who} trains with Adam only (got optimizer={c.get('optimizer')!r})")
        extra = set(c.get('optimizer_kwargs', {}) or {}) - {'betas', 'eps', 'weight_decay'}
        if extra:
            raise ValueError(f"{who}'s Adam takes betas / eps / weight_decay only (got {sorted(extra)})")
        if not c.get('epoch_call', True):
            raise ValueError(f"{who} issues each epoch from one host call: epoch_call=False is not supported")
        if c.get('skip_completed', False):
            raise ValueError(f"{who} trains every member: skip_completed is not supported")
    return configs


def check_shared(configs, free, what='one ensemble'):
    """Raise ValueError if two configs differ in a key outside `free`."""
    ref = configs[0]
    for i, c in enumerate(configs[1:], 1):
        for k in sorted((set(ref) | set(c)) - set(free)):
            if ref.get(k) != c.get(k):
                raise ValueError(f"config {i} differs from config 0 in {k!r} ({c.get(k)!r} vs {ref.get(k)!r}): members of "
                                 f"{what} may differ only in {sorted(free)}")


def validate_configs(configs):
    """Raise ValueError unless `configs` can train as one ensemble.  Touches no device."""
    configs = check_supported(configs)
    free = set(MEMBER_KEYS) | ({'scale_coeff'} if model_setting(configs[0], 'if_trainable_freq') else set())
    check_shared(configs, free)
    return configs


def sweep_data(configs, data_dicts):
    """One data dict per member: `data_dicts` is one dict (shared) or a list of len(configs).  Every member's train arrays
    must have the same shapes (one schedule for all); test sets may differ."""
    if isinstance(data_dicts, dict):
        return [data_dicts] * len(configs)
    datas = list(data_dicts)
    if len(datas) != len(configs):
        raise ValueError(f"{len(datas)} data dicts for {len(configs)} configs: give one dict, or one per config")
    ref = datas[0]
    for i, d in enumerate(datas[1:], 1):
        keys = sorted(k for k in set(ref) | set(d) if k.startswith('train_'))
        for k in keys:
            if k not in ref or k not in d or np.shape(ref[k]) != np.shape(d[k]):
                raise ValueError(f"data dict {i}'s {k!r} has shape {np.shape(d.get(k))}, data dict 0's "
                                 f"{np.shape(ref.get(k))}: every member trains on arrays of one shape")
    return datas


class EnsembleSolver:
    """R PTSolver runs of one configuration, trained together (see the module docstring).  The member solver of every kind:
    a kind is its validator, the _lib entry of one epoch and the form of that entry's arguments."""
    entry = 'model_ensemble_train_steps'
    per_member = False       # whether `entry` takes a MemberHParams and a ham_diag row per member (else one lr, one read-out)
    takes_descs = False      # whether `entry` takes the members' descriptors (else one, self.desc)

    def __init__(self, configs, data_dict, device=None, log=print):
        self.configs = validate_configs(configs)
        self._build([data_dict] * len(self.configs), device, log)

    def _build(self, data_dicts, device, log):
        """one PTSolver per member (member m on data_dicts[m]), their parameters and Adam moments as rows of [R, P] tensors"""
        self.device = device if device is not None else torch.device('cuda')
        if self.device.type != 'cuda':
            raise RuntimeError("EnsembleSolver runs on a HIP device only (no CPU fallback)")
        if any(c.get('train_noise') is not None for c in self.configs):
            # the member launches train the ideal circuit; a member that silently ignored its noise would be a wrong run
            raise ValueError(f"{type(self).__name__}: config key train_noise is not supported in member launches "
                             "(noise-aware training runs one model per PTSolver)")
        if any(c.get('train_noise_exact') is not None for c in self.configs):
            raise ValueError(f"{type(self).__name__}: config key train_noise_exact is not supported in member launches "
                             "(noise-aware training runs one model per PTSolver)")
        if any(c.get('train_device_noise') is not None for c in self.configs):
            raise ValueError(f"{type(self).__name__}: config key train_device_noise is not supported in member launches "
                             "(training under a DeviceNoise runs one model per PTSolver)")
        if any(c.get('train_device_noise_exact') is not None for c in self.configs):
            raise ValueError(f"{type(self).__name__}: config key train_device_noise_exact is not supported in member launches "
                             "(training under a DeviceNoise runs one model per PTSolver)")
        if any(c.get('train_sampling') is not None for c in self.configs):
            raise ValueError(f"{type(self).__name__}: config key train_sampling is not supported in member launches "
                             "(sampled-trajectory training runs one model per PTSolver)")
        if any(c.get('train_trajectories') is not None for c in self.configs):
            raise ValueError(f"{type(self).__name__}: config key train_trajectories is not supported in member launches "
                             "(sampled-trajectory training runs one model per PTSolver)")
        if any(c.get('train_jump_trajectories') is not None for c in self.configs):
            raise ValueError(f"{type(self).__name__}: config key train_jump_trajectories is not supported in member launches "
                             "(quantum-jump training runs one model per PTSolver)")
        self.log = log
        self.members = []
        for c, d in zip(self.configs, data_dicts):
            if c.get('seed') is not None:
                torch.manual_seed(int(c['seed']))
            self.members.append(PTSolver(c, d, device=self.device, log=lambda *a, **k: None))
        tr0 = self.members[0].trainer
        if tr0.desc is None or not tr0.epoch_call:
            raise RuntimeError("EnsembleSolver needs the fused model-level training path (QuanONetPT / HEAQNNPT in fp64)")
        self.desc = tr0.desc
        # the members' flat parameter vectors and Adam moments become rows of [R, P] tensors: one pointer per array for the
        # ensemble call, and every member's module, optimizer and checkpoints keep working on their row (members of a depth
        # sweep differ in size: member m's vector is the front of its row of [R, Pmax])
        R = len(self.members)
        self.numels = [m.trainer.numel for m in self.members]
        P = max(self.numels)
        self.params = torch.zeros(R, P, dtype=torch.float64, device=self.device)
        for i, m in enumerate(self.members):
            self.params[i, :self.numels[i]].copy_(m.trainer.pflat)
        self.exp_avg = torch.zeros(R, P, dtype=torch.float64, device=self.device)
        self.exp_avg_sq = torch.zeros(R, P, dtype=torch.float64, device=self.device)
        for i, m in enumerate(self.members):
            tr = m.trainer
            tr.pflat = self.params[i, :self.numels[i]]
            off = 0
            for p in tr.params:
                p.data = tr.pflat[off:off + p.numel()].view(p.shape)
                off += p.numel()
            tr.optimizer.pflat = tr.pflat
            tr.optimizer.exp_avg = self.exp_avg[i, :self.numels[i]]
            tr.optimizer.exp_avg_sq = self.exp_avg_sq[i, :self.numels[i]]
        self.rngs = [np.random.RandomState(c.get('seed')) for c in self.configs]

    def _stage_epoch(self, n, bs, nb):
        """Every member's batch order for one epoch and its rows gathered in that order, as [R, n, ...] blocks."""
        m0 = self.members[0]
        idx = [torch.as_tensor(rs.permutation(n), device=self.device) for rs in self.rngs]
        inputs = [torch.stack([m.train_input[k][i] for m, i in zip(self.members, idx)]) for k in range(len(m0.train_input))]
        out = torch.stack([m.train_output[i] for m, i in zip(self.members, idx)]).reshape(len(idx), n)
        return inputs, out

    def train(self):
        """Train every member for num_epochs; returns the list of their history dicts."""
        from . import _lib
        m0 = self.members[0]
        R = len(self.members)
        n = m0.train_output.shape[0]
        bs = min(int(m0.config.get('batch_size', 100)), n)
        epochs = int(m0.config['num_epochs'])
        nb, gbs, bounds = batch_plan(n, bs)
        nm = max(self.numels)
        histories = [{'loss_train': [], 'loss_test': []} for _ in range(R)]
        want_save = m0.config.get('if_save', True)
        for m in self.members:
            os.makedirs(m.out_dir, exist_ok=True)
            m.best_model_path = os.path.join(m.out_dir, 'best_model.pt')
        opt0 = m0.trainer.optimizer

        def stage():
            return self._stage_epoch(n, bs, nb)

        def issue(staged):
            """queue one epoch's steps of every member; returns the device rows of their [sse | sum y^2]"""
            for m in self.members:
                m.model.train()
            inputs, out = staged
            rows = torch.zeros(R, nb, nm + 2, dtype=torch.float64, device=self.device)
            self._train_steps(bounds, gbs, inputs, out, rows, opt0.t + 1)
            for m in self.members:
                m.trainer.optimizer.t += nb
            if all(p == nm for p in self.numels):
                return rows[:, :, nm:], None
            return torch.stack([rows[r, :, p:p + 2] for r, p in enumerate(self.numels)]), None   # member r's [sse | sum y^2]

        def record(epoch, tl, snap):
            for r, m in enumerate(self.members):                # member r's accounting is its PTSolver's
                m._record_epoch(epoch, histories[r], tl[r], gbs, snap[r] if want_save else None, want_save, self.log,
                                tag=f"[{m.config.get('run_id', r)}] ")

        run_epochs(epochs, stage() if epochs > 0 else None, stage, issue, lambda: _lib.check_status(self.device),
                   lambda _: self.params.detach().to('cpu', copy=True) if want_save else None,
                   [m.lr_scheduler for m in self.members if m.lr_scheduler is not None], record)
        if want_save:
            for m in self.members:
                m._save(os.path.join(m.out_dir, 'final.pt'))
        return histories

    def _hparam_rows(self):
        """every member's read-out, scale and CURRENT learning rate (its scheduler has stepped)"""
        from . import _lib
        return [_lib.member_hparams(d.scale_coeff, d.ham_offset, d.ham_coeff, m.trainer.optimizer.hparams()[0], d.ham_pauli)
                for m, d in zip(self.members, self.descs)]

    def _train_steps(self, bounds, gbs, inputs, out, rows, first_step):
        """one epoch's steps of every member, one launch per kernel and step"""
        from . import _lib
        m0 = self.members[0]
        lr, *adam = m0.trainer.optimizer.hparams()
        call = (bounds, gbs, *split_inputs(inputs), out, self.params, rows, self.exp_avg, self.exp_avg_sq, first_step)
        if self.per_member:
            getattr(_lib, self.entry)(self.descs if self.takes_descs else self.desc, self._hparam_rows(), *call, *adam,
                                      ham_diag=self.ham_diag)
        else:
            getattr(_lib, self.entry)(self.desc, *call, lr, *adam, ham_diag=m0.trainer._ham_diag())

    def predict(self, inputs, batch_size=None):
        """Every member's predictions on the same inputs (the single-model forward path), as a list."""
        return [m.predict(inputs, batch_size=batch_size) for m in self.members]

    def evaluate(self, histories=None):
        """PTSolver.evaluate for every member (its best checkpoint, its metric.json); returns the list of metrics."""
        histories = histories if histories is not None else [None] * len(self.members)
        return [m.evaluate(h) for m, h in zip(self.members, histories)]

    def evaluate_noisy(self, noise, out_name=None, exact=False, sampling=None):
        """PTSolver.evaluate_noisy for every member (its best checkpoint; out_dir/out_name when given, never metric.json); returns
        the list of results.  Every member uses noise.seed, so the members see common random numbers: member differences are
        not blurred by independent noise draws.  exact=True (or 'wide', which reaches n = 9, or 'device': a DeviceNoise up to
        n = 9): every member's exact expectation instead (no draws at all); a
        quanonet_amd.noise.DeviceNoise is evaluated that way, or sampled with sampling= (one Sampling, so one seed, for every
        member: common random numbers again); ValueError with neither."""
        return [m.evaluate_noisy(noise, out_name, exact=exact, sampling=sampling) for m in self.members]


class PerMemberSolver(EnsembleSolver):
    """The kinds whose members carry hyper-parameters of their own: SweepSolver, DepthSweepSolver, QubitSweepSolver.  A kind
    sets `validate` (its validate_*_configs), `entry` and `takes_descs`."""
    per_member = True
    validate = None

    def __init__(self, configs, data_dicts, device=None, log=print):
        self.configs = type(self).validate(configs, data_dicts)
        self._build(sweep_data(self.configs, data_dicts), device, log)
        self.descs = [m.trainer.desc for m in self.members]
        if any(d is None for d in self.descs):
            raise RuntimeError(f"{type(self).__name__} needs the fused model-level training path (QuanONetPT / HEAQNNPT in fp64)")
        diags = [m.trainer._ham_diag() for m in self.members]
        self.ham_diag = None
        if diags[0] is not None:            # [R, 2^nmax]: member m's spectrum at the front of row m
            width = max(d.numel() for d in diags)
            self.ham_diag = torch.zeros(len(diags), width, dtype=torch.float64, device=self.device)
            for i, d in enumerate(diags):
                self.ham_diag[i, :d.numel()].copy_(d.reshape(-1))
