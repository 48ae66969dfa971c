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

from .solver import PTSolver

# keys in which the members of one ensemble may differ (scale_coeff too, for trainable-frequency models: there it only sets
# the initial frequency weights, the descriptor the kernels see is shared)
MEMBER_KEYS = ('seed', 'run_id', 'prefix')


def _trainable(cfg):
    return str(cfg.get('if_trainable_freq', 'true')).lower() == 'true'


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
    free = set(MEMBER_KEYS) | ({'scale_coeff'} if _trainable(configs[0]) else set())
    check_shared(configs, free)
    return configs


class EnsembleSolver:
    """R PTSolver runs of one configuration, trained together (see the module docstring)."""

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
        nb = max(1, int(np.ceil(n / bs)))
        bounds = [min(i * bs, n) for i in range(nb)] + [n]
        gbs = [min(bs, n - i * bs) for i in range(nb)]
        nm = max(self.numels)
        histories = [{'loss_train': [], 'loss_test': []} for _ in range(R)]
        want_save = m0.config.get('if_save', True)
        for m in self.members:
            os.makedirs(m.out_dir, exist_ok=True)
            m.best_model_path = os.path.join(m.out_dir, 'best_model.pt')
        opt0 = m0.trainer.optimizer

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
                return rows[:, :, nm:]
            return torch.stack([rows[r, :, p:p + 2] for r, p in enumerate(self.numels)])   # member r's [sse | sum y^2]

        cur = issue(self._stage_epoch(n, bs, nb)) if epochs > 0 else None
        for epoch in range(epochs):
            tails = cur
            staged = self._stage_epoch(n, bs, nb) if epoch + 1 < epochs else None
            tl = tails.tolist()                                 # one host sync per epoch
            _lib.check_status(self.device)                      # a kernel-side pipeline failure ends the run here
            snap = self.params.detach().to('cpu', copy=True) if want_save else None
            for m in self.members:                              # (the schedulers depend on the epoch count alone)
                if m.lr_scheduler is not None:
                    m.lr_scheduler.step()
            cur = issue(staged) if staged is not None else None
            for r, m in enumerate(self.members):
                s = [0.0, 0.0, 0.0]                             # as PTSolver.train: batch MSE, sse, sum y^2 in step order
                for i in range(nb):
                    s[0] += tl[r][i][0] / gbs[i]
                    s[1] += tl[r][i][0]
                    s[2] += tl[r][i][1]
                avg_loss = s[0] / nb
                histories[r]['loss_train'].append(avg_loss)
                if avg_loss < m.best_loss:
                    m.best_loss = avg_loss
                    if want_save:
                        m._save(m.best_model_path, flat=snap[r])
                if epoch % 10 == 0:
                    avg_rel = np.sqrt(s[1]) / (np.sqrt(s[2]) + 1e-8)
                    self.log(f"[{m.config.get('run_id', r)}] Epoch {epoch} | MSE: {avg_loss:.6e} | Rel_L2: {avg_rel:.4%}")
        if want_save:
            for m in self.members:
                m._save(os.path.join(m.out_dir, 'final.pt'))
        return histories

    def _train_steps(self, bounds, gbs, inputs, out, rows, first_step):
        """one epoch's steps of every member, one launch per kernel and step"""
        from . import _lib
        m0 = self.members[0]
        g = m0.trainer.optimizer.param_groups[0]
        _lib.model_ensemble_train_steps(self.desc, bounds, gbs, inputs[0], inputs[1] if len(inputs) > 1 else None, out,
                                        self.params, rows, self.exp_avg, self.exp_avg_sq, first_step, g['lr'],
                                        g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'],
                                        ham_diag=m0.trainer._ham_diag())

    def predict(self, inputs, batch_size=None):
        """Every member's predictions on the same inputs (the single-model forward path), as a list."""
        return [m.predict(inputs, batch_size=batch_size) for m in self.members]

    def evaluate(self, histories=None):
        """PTSolver.evaluate for every member (its best checkpoint, its metric.json); returns the list of metrics."""
        histories = histories if histories is not None else [None] * len(self.members)
        return [m.evaluate(h) for m, h in zip(self.members, histories)]

    def evaluate_noisy(self, noise, out_name=None, exact=False):
        """PTSolver.evaluate_noisy for every member (its best checkpoint; out_dir/out_name when given, never metric.json); returns
        the list of results.  Every member uses noise.seed, so the members see common random numbers: member differences are
        not blurred by independent noise draws.  exact=True: every member's exact expectation instead (no draws at all); a
        quanonet_amd.noise.DeviceNoise is evaluated that way only (ValueError with exact=False)."""
        return [m.evaluate_noisy(noise, out_name, exact=exact) for m in self.members]
