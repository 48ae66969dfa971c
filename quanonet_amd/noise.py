"""
Evaluation of trained models under gate noise, readout error and finite shots (qhea_model_forward_noisy, n <= 12): the deployment
questions of the reference's ibm_inference.py -- how many shots a model needs, what gate error rate it tolerates -- answered
on the GPU before any QPU time is spent.  The noise model, the estimators and the random-number layout are stated in
include/quanonet_hea.h.
"""
import dataclasses
from dataclasses import dataclass

import torch

from . import _lib


@dataclass(frozen=True)
class NoiseModel:
    """
    p1: depolarizing probability after every single-qubit gate (each encoding RX; each wire's RY RZ RY counts as one gate);
    p2: two-qubit depolarizing probability after every CNOT; readout: flip probability of every measured bit.
    shots = 0: expectation mode, the mean over `trajectories` noisy runs of their exact read-outs (readout error folded in);
    shots = S >= 1: S sampled bitstrings per row, what an Estimator with default_shots = S estimates.
    seed: key of the counter-based random streams; a row's draws depend on (seed, global row index, trajectory) only.
    """
    p1: float = 0.0
    p2: float = 0.0
    readout: float = 0.0
    shots: int = 0
    trajectories: int = 1
    seed: int = 0

    def __post_init__(self):
        for name in ('p1', 'p2', 'readout'):
            v = getattr(self, name)
            if not isinstance(v, (int, float)) or not 0.0 <= float(v) <= 1.0:
                raise ValueError(f"NoiseModel.{name} must lie in [0, 1] (got {v!r})")
        for name in ('shots', 'trajectories', 'seed'):
            if not isinstance(getattr(self, name), int) or isinstance(getattr(self, name), bool):
                raise ValueError(f"NoiseModel.{name} must be an int (got {getattr(self, name)!r})")
        if self.shots < 0:
            raise ValueError(f"NoiseModel.shots must be >= 0 (got {self.shots})")
        if self.shots == 0 and self.trajectories < 1:
            raise ValueError(f"NoiseModel.trajectories must be >= 1 in expectation mode (got {self.trajectories})")
        if not 0 <= self.seed < 1 << 64:
            raise ValueError(f"NoiseModel.seed must fit in 64 unsigned bits (got {self.seed})")

    def params(self):
        """The C ABI's qhea_noise."""
        return _lib.NoiseParams(float(self.p1), float(self.p2), float(self.readout), int(self.shots), int(self.trajectories),
                                int(self.seed))

    def asdict(self):
        return dataclasses.asdict(self)


def _model_inputs(model, inputs):
    ins = list(inputs) if isinstance(inputs, (tuple, list)) else [inputs]
    ins = [t.contiguous() for t in ins]
    return ins[0], (ins[1] if len(ins) > 1 else None)


def _call_args(model, inputs, who):
    """(desc, flat parameters, ham_diag, branch, trunk) of a fp64 model on a HIP device, as the C ABI takes them"""
    if not hasattr(model, 'fused_desc'):
        raise TypeError(f"{who} takes a QuanONetPT or HEAQNNPT model")
    params = list(model.parameters())
    if not params or params[0].dtype != torch.float64 or not params[0].is_cuda:
        raise _lib.QheaError(f"{who} needs a float64 model on a HIP device (there is no CPU path)")
    desc = model.fused_desc()
    flat = torch.cat([p.detach().reshape(-1) for p in params])
    if flat.numel() != _lib.model_param_count(desc):
        raise _lib.QheaError("the model's parameters do not match the flat layout of its descriptor")
    q = getattr(model, 'quantum_layer', None)
    ham_diag = q.ham_diag if (q is not None and getattr(q, 'use_full_ham', False)) else None
    if ham_diag is not None:
        ham_diag = ham_diag.detach().to(torch.float64).contiguous()
    branch, trunk = _model_inputs(model, inputs)
    return desc, flat, ham_diag, branch, trunk


def noisy_predict(model, inputs, noise, chunk_rows=16384, row0=0):
    """
    Predictions of a fp64 QuanONetPT / HEAQNNPT on a HIP device under `noise` (a NoiseModel): (pred [N, 1], stderr [N]).
    inputs: (branch, trunk) for QuanONet, (x,) or x for HEAQNN.  Rows go in chunks of `chunk_rows`; chunk i passes its global
    index row0 + i * chunk_rows, so the result is bitwise the same for any chunking.  Parameters in model.parameters() order
    (the flat layout of the header), ham_diag as the trainer takes it.  n <= 6 runs qhea_model_forward_noisy, n = 7..12
    qhea_model_forward_noisy_wide: one quantity, one random stream, one code path per n.
    """
    desc, flat, ham_diag, branch, trunk = _call_args(model, inputs, 'noisy_predict')
    N = branch.shape[0]
    pred = torch.empty(N, dtype=torch.float64, device=branch.device)
    stderr = torch.empty(N, dtype=torch.float64, device=branch.device)
    chunk = max(1, int(chunk_rows))
    nz = noise.params()
    forward = _lib.model_forward_noisy_wide if desc.n_qubits >= 7 else _lib.model_forward_noisy
    for s in range(0, N, chunk):
        e = min(N, s + chunk)
        forward(desc, branch[s:e], None if trunk is None else trunk[s:e], flat, nz, row0=int(row0) + s, ham_diag=ham_diag,
                out=pred[s:e], stderr=stderr[s:e])
    return pred.unsqueeze(-1), stderr


def exact_noisy_predict(model, inputs, noise, chunk_rows=16384):
    """
    The exact counterpart of noisy_predict (qhea_model_forward_noisy_exact): (pred [N, 1], shot_std [N]) -- each row's exact
    expectation under `noise` (its p1, p2 and readout; shots, trajectories and seed are ignored) and the exact standard
    deviation of one shot, so that a row's standard error at S shots is shot_std / sqrt(S).  No sampling error, no random
    numbers; n <= 6.  Rows go in chunks of `chunk_rows`; the result is bitwise the same for any chunking.
    """
    desc, flat, ham_diag, branch, trunk = _call_args(model, inputs, 'exact_noisy_predict')
    N = branch.shape[0]
    pred = torch.empty(N, dtype=torch.float64, device=branch.device)
    shot_std = torch.empty(N, dtype=torch.float64, device=branch.device)
    chunk = max(1, int(chunk_rows))
    nz = noise.params()
    for s in range(0, N, chunk):
        e = min(N, s + chunk)
        _lib.model_forward_noisy_exact(desc, branch[s:e], None if trunk is None else trunk[s:e], flat, nz, ham_diag=ham_diag,
                                       out=pred[s:e], shot_std=shot_std[s:e])
    return pred.unsqueeze(-1), shot_std


def amplification(model, noise):
    """
    log10 of the factor by which the gradient's inverse walk amplifies the traceless part of rho for this model's circuit
    under `noise`: (1 - 4 p1 / 3)^-L1 (1 - 16 p2 / 15)^-L2 over its L1 one-qubit and L2 CNOT noise locations.  The noise-aware
    training calls refuse values above 12 (and singular channels, inf); no device is needed.
    """
    if not hasattr(model, 'fused_desc'):
        raise TypeError("amplification takes a QuanONetPT or HEAQNNPT model")
    return _lib.model_exact_noisy_log10_amplification(model.fused_desc(), noise.params())


def exact_noisy_loss_and_grad(model, inputs, y, noise, inv_batch_total=None):
    """
    The MSE loss of the exact noisy prediction (exact_noisy_predict) and its exact gradient, as the flat [P + 2] tensor of
    qhea_model_loss_grad_noisy_exact: d/dparams of sum_b (pred_b - y_b)^2 * inv_batch_total in model.parameters() order, then
    sum (pred - y)^2 and sum y^2.  inv_batch_total defaults to 1 / rows (the mean); a shard of a larger batch passes the global
    value.  The gradient is computed by the adjoint walk through the density matrix: no sampling, n <= 6.
    """
    desc, flat, ham_diag, branch, trunk = _call_args(model, inputs, 'exact_noisy_loss_and_grad')
    B = branch.shape[0]
    y = y.detach().to(torch.float64).reshape(-1).contiguous()
    grad = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=branch.device)
    if B == 0:
        return grad
    inv = 1.0 / B if inv_batch_total is None else float(inv_batch_total)
    return _lib.model_loss_grad_noisy_exact(desc, branch, trunk, y, flat, noise.params(), inv, grad, ham_diag=ham_diag)
