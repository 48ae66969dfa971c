"""
Evaluation of trained models under gate noise, readout error and finite shots (qhea_model_forward_noisy, n <= 12): the deployment
questions of the reference's ibm_inference.py -- how many shots a model needs, what gate error rate it tolerates -- answered
on the GPU before any QPU time is spent.  The noise model, the estimators and the random-number layout are stated in
include/quanonet_hea.h.
"""
import ctypes
import dataclasses
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .solver import split_inputs


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


@dataclass(frozen=True)
class Sampling:
    """
    The estimator of device_noisy_predict (qhea_sampling): shots = 0 is expectation mode, the mean over `trajectories`
    quantum-jump runs of their exact read-outs (readout error folded in); shots = S >= 1 draws S bitstrings per row, what an
    Estimator with default_shots = S estimates.  seed: key of the counter-based random streams; a row's draws depend on
    (seed, global row index, trajectory) only.
    """
    shots: int = 0
    trajectories: int = 1
    seed: int = 0

    def __post_init__(self):
        for name in ('shots', 'trajectories', 'seed'):
            if not isinstance(getattr(self, name), int) or isinstance(getattr(self, name), bool):
                raise ValueError(f"Sampling.{name} must be an int (got {getattr(self, name)!r})")
        if self.shots < 0:
            raise ValueError(f"Sampling.shots must be >= 0 (got {self.shots})")
        if self.shots == 0 and self.trajectories < 1:
            raise ValueError(f"Sampling.trajectories must be >= 1 in expectation mode (got {self.trajectories})")
        if not 0 <= self.seed < 1 << 64:
            raise ValueError(f"Sampling.seed must fit in 64 unsigned bits (got {self.seed})")

    def params(self):
        """The C ABI's qhea_sampling."""
        return _lib.SamplingParams(int(self.shots), int(self.trajectories), int(self.seed))

    def asdict(self):
        return dataclasses.asdict(self)


_PER_WIRE = ('p1', 'p2', 'readout01', 'readout10', 't1', 't2')
_DURATIONS = ('t_rx', 't_rot', 't_cx')


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


@dataclass(frozen=True)
class DeviceNoise:
    """
    The calibrated device noise model of qhea_device_noise (include/quanonet_hea.h), for the exact evaluation
    (exact_noisy_predict, evaluate_noisy(exact=True)); n <= 6 (device_exact_noisy_predict, evaluate_noisy(exact='device'); n <= 9),
    and for quantum-jump trajectories (device_noisy_predict, evaluate_noisy(sampling=...)); n <= 12.
    p1[q]: depolarizing probability after every single-qubit gate on wire q; p2[j]: two-qubit depolarizing probability after
    the CNOT of ring slot j (control (j+1) mod n -> target j); readout01[q] / readout10[q]: probability that bit q reads 1
    given 0 / 0 given 1; t1[q], t2[q]: relaxation times of wire q (math.inf: no decay; t2 <= 2 t1).  Each of the six is one
    float for every wire or a sequence with one entry per wire.  t_rx, t_rot, t_cx: durations of the encoding layer, the
    rotation layer and one CNOT slot, in the unit of t1 / t2.  idle: wires outside a CNOT slot relax during it (the ring is
    sequential, so a sub-layer lasts n slots).  The defaults are the ideal circuit.
    """
    p1: object = 0.0
    p2: object = 0.0
    readout01: object = 0.0
    readout10: object = 0.0
    t1: object = math.inf
    t2: object = math.inf
    t_rx: float = 0.0
    t_rot: float = 0.0
    t_cx: float = 0.0
    idle: bool = True

    def __post_init__(self):
        for name in _PER_WIRE:
            v = getattr(self, name)
            if not _number(v):
                try:
                    v = tuple(v)
                except TypeError:
                    v = (v,)
                if not v or not all(_number(x) for x in v):
                    raise ValueError(f"DeviceNoise.{name} must be a number or a non-empty sequence of numbers "
                                     f"(got {getattr(self, name)!r})")
                v = tuple(float(x) for x in v)
                object.__setattr__(self, name, v)
            for x in (v if isinstance(v, tuple) else (v,)):
                if name in ('t1', 't2'):
                    if not x > 0.0:
                        raise ValueError(f"DeviceNoise.{name} must be > 0 (got {x!r})")
                elif not 0.0 <= x <= 1.0:
                    raise ValueError(f"DeviceNoise.{name} must lie in [0, 1] (got {x!r})")
        lengths = {len(getattr(self, name)) for name in _PER_WIRE if isinstance(getattr(self, name), tuple)}
        if len(lengths) > 1:
            raise ValueError(f"DeviceNoise: the per-wire sequences differ in length ({sorted(lengths)})")
        wires = lengths.pop() if lengths else 1
        for q in range(wires):
            if self._at('t2', q) > 2.0 * self._at('t1', q):
                raise ValueError(f"DeviceNoise: t2 must not exceed 2 t1 (wire {q}: t1 = {self._at('t1', q)!r}, "
                                 f"t2 = {self._at('t2', q)!r})")
        for name in _DURATIONS:
            v = getattr(self, name)
            if not _number(v) or not 0.0 <= v < math.inf:
                raise ValueError(f"DeviceNoise.{name} must be a finite duration >= 0 (got {v!r})")
        if not isinstance(self.idle, bool):
            raise ValueError(f"DeviceNoise.idle must be a bool (got {self.idle!r})")

    def _at(self, name, q):
        v = getattr(self, name)
        return v[q] if isinstance(v, tuple) else float(v)

    def _wires(self, name, n):
        v = getattr(self, name)
        if isinstance(v, tuple):
            if len(v) != n:
                raise ValueError(f"DeviceNoise.{name} has {len(v)} entries, the circuit has {n} wires")
            return v
        return (float(v),) * n

    def params(self, n):
        """The C ABI's qhea_device_noise for an n-qubit circuit (the record keeps its six arrays alive)."""
        n = int(n)
        arrays = [(ctypes.c_double * n)(*self._wires(name, n)) for name in _PER_WIRE]
        f64p = ctypes.POINTER(ctypes.c_double)
        rec = _lib.DeviceNoiseParams(n, 1 if self.idle else 0, *[ctypes.cast(a, f64p) for a in arrays], float(self.t_rx),
                                     float(self.t_rot), float(self.t_cx))
        rec._arrays = arrays
        return rec

    def tables(self, n):
        """(chan [4, n, 3], lam2 [n]) of qhea_device_noise_tables: the (off, a, b) triple of every channel site (ENC, ROT, CTL,
        TGT) and wire, with the idle decay folded in, and 16 p2[j] / 15 per CNOT slot.  No device needed."""
        return _lib.device_noise_tables(n, self.params(n))

    def jump_tables(self, n):
        """jump [4, n, 2] of qhea_device_noise_jump_tables: (gamma, pz) of the relaxation of every channel site (ENC, ROT, CTL,
        TGT) and wire at its folded duration -- damping probability and dephasing probability of the trajectory unravelling.
        No device needed."""
        return _lib.device_noise_jump_tables(n, self.params(n))

    def asdict(self):
        """JSON-serialisable (json.dumps(..., allow_nan=False) accepts it): per-wire sequences as lists, an infinite t1 / t2
        as the string 'Infinity' -- what float() reads back, so DeviceNoise.fromdict(json.loads(...)) restores the setting."""
        def enc(v):
            if isinstance(v, tuple):
                return [enc(x) for x in v]
            return 'Infinity' if isinstance(v, float) and math.isinf(v) else v
        return {f.name: enc(getattr(self, f.name)) for f in dataclasses.fields(self)}

    @classmethod
    def fromdict(cls, d):
        """The inverse of asdict."""
        def dec(v):
            if isinstance(v, (list, tuple)):
                return tuple(dec(x) for x in v)
            return float(v) if isinstance(v, str) else v
        return cls(**{k: dec(v) for k, v in d.items()})

    @classmethod
    def uniform(cls, noise_model):
        """The NoiseModel's channels as a DeviceNoise: its p1 on every wire, its p2 in every slot, its symmetric readout flip in
        both directions, no relaxation.  (shots, trajectories and seed have no counterpart: the evaluation is exact.)"""
        return cls(p1=float(noise_model.p1), p2=float(noise_model.p2), readout01=float(noise_model.readout),
                   readout10=float(noise_model.readout))

    @classmethod
    def from_calibration(cls, cal, wires, pulses_rx=2, pulses_rot=2, idle=True):
        """
        The model for the ring placed on the physical qubits `wires` (wire q of the circuit = qubit wires[q]), from a plain
        dict of the quantities the reference's profile_hardware reads from a backend:
          cal['qubits'][str(k)]: 'T1', 'T2', 'sx_error', 'sx_length', and 'readout_error' or the pair 'prob_meas1_prep0' /
                                 'prob_meas0_prep1' (the pair wins where both are given);
          cal['pairs']['a_b']:   'gate_error', 'gate_length' of the two-qubit gate on qubits a and b, either order.
        Average gate infidelities r become this project's depolarizing probabilities: p = 3 r / 2 for one qubit, p = 5 r / 4 for
        two.  A layer of `pulses` sx pulses has p1 = 1 - (1 - p_sx)^pulses and lasts pulses * sx_length (the longest of the
        wires: the layer is one event on every wire at once); t_cx is the longest gate_length on the ring.  pulses_rx and
        pulses_rot must be equal (ValueError otherwise): the model has one p1 per wire for both of its layers, so two pulse
        counts would have no setting that states them.  `idle` is DeviceNoise.idle.  All times in the unit the calibration
        uses.  A ring edge without a calibrated pair raises ValueError.  T2 above 2 T1 (a calibration can report it within
        its error bars) is clipped.
        """
        wires = [int(k) for k in wires]
        n = len(wires)
        if n < 2 or len(set(wires)) != n:
            raise ValueError(f"from_calibration: wires must name at least two distinct qubits (got {wires})")
        qubits, pairs = cal.get('qubits', {}), cal.get('pairs', {})
        per = []
        for k in wires:
            if str(k) not in qubits:
                raise ValueError(f"from_calibration: qubit {k} is not in the calibration")
            per.append(qubits[str(k)])
        slots = []
        for j in range(n):                                               # slot j: control wires[(j + 1) % n] -> target wires[j]
            a, b = wires[(j + 1) % n], wires[j]
            edge = pairs.get(f'{a}_{b}', pairs.get(f'{b}_{a}'))
            if edge is None:
                raise ValueError(f"from_calibration: ring edge ({a}, {b}) has no calibrated two-qubit gate; choose wires whose "
                                 "ring is native on the device (routing is out of scope)")
            slots.append(edge)

        def layer_p1(c, pulses):
            return 1.0 - (1.0 - min(1.0, 1.5 * float(c['sx_error']))) ** int(pulses)
        if pulses_rx != pulses_rot:
            # one p1 per wire in the model: a wire's two layers must compile to the same number of pulses
            raise ValueError("from_calibration: pulses_rx and pulses_rot must be equal (the model has one p1 per wire)")
        sx_len = max(float(c['sx_length']) for c in per)
        r01 = [float(c.get('prob_meas1_prep0', c.get('readout_error', 0.0))) for c in per]
        r10 = [float(c.get('prob_meas0_prep1', c.get('readout_error', 0.0))) for c in per]
        t1 = [float(c['T1']) for c in per]
        t2 = [min(float(c['T2']), 2.0 * float(c['T1'])) for c in per]
        return cls(p1=[layer_p1(c, pulses_rx) for c in per], p2=[min(1.0, 1.25 * float(e['gate_error'])) for e in slots],
                   readout01=r01, readout10=r10, t1=t1, t2=t2, t_rx=int(pulses_rx) * sx_len, t_rot=int(pulses_rot) * sx_len,
                   t_cx=max(float(e['gate_length']) for e in slots), idle=idle)


def _uniform_only(noise, who, why):
    if isinstance(noise, DeviceNoise):
        raise ValueError(f"{who} takes a NoiseModel, not a DeviceNoise: {why}; device_noisy_predict and "
                         "evaluate_noisy(noise, sampling=Sampling(...)) sample a DeviceNoise by quantum-jump trajectories, "
                         "exact_noisy_predict and evaluate_noisy(exact=True) evaluate one exactly, device_noisy_loss_and_grad, "
                         "device_amplification and the config key train_device_noise differentiate and train under one")


_TRAJECTORY_WHY = ("this call's trajectory kernels sample Pauli errors only and relaxation is not a Pauli channel: a DeviceNoise "
                   "goes to device_noisy_predict, or to evaluate_noisy with the sampling= argument")
_GRADIENT_WHY = "this call's reverse walk inverts the uniform depolarizing channels only"


def _model_inputs(model, inputs):
    ins = list(inputs) if isinstance(inputs, (tuple, list)) else [inputs]
    return split_inputs([t.contiguous() for t in ins])


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
    _uniform_only(noise, 'noisy_predict', _TRAJECTORY_WHY)
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


def device_noisy_predict(model, inputs, noise, sampling, chunk_rows=16384, row0=0):
    """
    noisy_predict under a DeviceNoise (qhea_model_forward_noisy_device for n = 2..9, qhea_model_forward_noisy_device_wide for
    n = 10..12; the same model, unravelling and random stream): (pred [N, 1], stderr [N]) from quantum-jump trajectories
    -- sampled Paulis for the gate errors, dephasing and norm-dependent damping jumps for T1 / T2 with the ring's idle decay,
    the asymmetric readout -- with the estimator `sampling` (a Sampling: expectation mode or shots, and the seed).  Unbiased for
    exact_noisy_predict(model, inputs, noise); n = 2..12.  Rows go in chunks of `chunk_rows`; chunk i passes its global index
    row0 + i * chunk_rows, so the result is bitwise the same for any chunking.
    """
    if not isinstance(noise, DeviceNoise):
        raise ValueError(f"device_noisy_predict takes a DeviceNoise (got {type(noise).__name__}); a NoiseModel goes to "
                         "noisy_predict, or through DeviceNoise.uniform")
    if not isinstance(sampling, Sampling):
        raise ValueError(f"device_noisy_predict takes a Sampling (got {type(sampling).__name__})")
    desc, flat, ham_diag, branch, trunk = _call_args(model, inputs, 'device_noisy_predict')
    N = branch.shape[0]
    pred = torch.empty(N, dtype=torch.float64, device=branch.device)
    stderr = torch.empty(N, dtype=torch.float64, device=branch.device)
    chunk = max(1, int(chunk_rows))
    nz, sp = noise.params(desc.n_qubits), sampling.params()
    forward = _lib.model_forward_noisy_device_wide if desc.n_qubits >= 10 else _lib.model_forward_noisy_device
    for s in range(0, N, chunk):
        e = min(N, s + chunk)
        forward(desc, branch[s:e], None if trunk is None else trunk[s:e], flat, nz, sp, row0=int(row0) + s, ham_diag=ham_diag,
                out=pred[s:e], stderr=stderr[s:e])
    return pred.unsqueeze(-1), stderr


def exact_noisy_predict(model, inputs, noise, chunk_rows=16384):
    """
    The exact counterpart of noisy_predict (qhea_model_forward_noisy_exact): (pred [N, 1], shot_std [N]) -- each row's exact
    expectation under `noise` (its p1, p2 and readout; shots, trajectories and seed are ignored) and the exact standard
    deviation of one shot, so that a row's standard error at S shots is shot_std / sqrt(S).  No sampling error, no random
    numbers; n <= 6.  Rows go in chunks of `chunk_rows`; the result is bitwise the same for any chunking.
    `noise` may also be a DeviceNoise: the same two quantities under the calibrated device model
    (qhea_model_forward_noisy_device_exact).
    """
    desc, flat, ham_diag, branch, trunk = _call_args(model, inputs, 'exact_noisy_predict')
    N = branch.shape[0]
    pred = torch.empty(N, dtype=torch.float64, device=branch.device)
    shot_std = torch.empty(N, dtype=torch.float64, device=branch.device)
    chunk = max(1, int(chunk_rows))
    if isinstance(noise, DeviceNoise):
        forward, nz = _lib.model_forward_noisy_device_exact, noise.params(desc.n_qubits)
    else:
        forward, nz = _lib.model_forward_noisy_exact, noise.params()
    for s in range(0, N, chunk):
        e = min(N, s + chunk)
        forward(desc, branch[s:e], None if trunk is None else trunk[s:e], flat, nz, ham_diag=ham_diag, out=pred[s:e],
                shot_std=shot_std[s:e])
    return pred.unsqueeze(-1), shot_std


# the density matrices of a default chunk of wide_exact_noisy_predict: 256 MiB, 17 % faster than 64 MiB and 1 GiB at n = 8 and 9
# (profiles/r37_exact_noisy_wide_rate.json, chunk_sweep)
WIDE_EXACT_STATE_BYTES = 1 << 28


def wide_exact_noisy_predict(model, inputs, noise, chunk_rows=None):
    """
    exact_noisy_predict for n = 2..9: (pred [N, 1], shot_std [N]).  n <= 6 is exact_noisy_predict itself (bitwise; a DeviceNoise
    is allowed there).  n = 7..9 runs qhea_model_forward_noisy_exact_wide, which keeps the density matrices of a chunk of rows in
    device memory, 4^n x 16 bytes per row, and takes a NoiseModel only (device_exact_noisy_predict is the call for a DeviceNoise
    at those sizes).  Rows go in chunks of the largest count whose density
    matrices stay within 256 MiB (1024 / 256 / 64 rows at n = 7 / 8 / 9), and of no more than `chunk_rows` when given; the
    result is bitwise the same for any chunking.
    """
    desc, flat, ham_diag, branch, trunk = _call_args(model, inputs, 'wide_exact_noisy_predict')
    n = desc.n_qubits
    if n <= 6:
        return exact_noisy_predict(model, inputs, noise) if chunk_rows is None else \
            exact_noisy_predict(model, inputs, noise, chunk_rows=chunk_rows)
    if n >= 10:
        raise ValueError(f"wide_exact_noisy_predict covers n = 2..9 (got n = {n}): a density matrix of 4^{n} elements per row "
                         "is not carried; noisy_predict estimates a NoiseModel at n = 10..12 from trajectories and "
                         "device_noisy_predict a DeviceNoise")
    if isinstance(noise, DeviceNoise):
        raise ValueError(f"wide_exact_noisy_predict evaluates a NoiseModel at n = 7..9 (got a DeviceNoise at n = {n}): the tiled "
                         "density-matrix kernels of this call carry the uniform channels only; exact_noisy_predict evaluates a "
                         "DeviceNoise exactly at n <= 6 and device_exact_noisy_predict at n <= 9, device_noisy_predict and "
                         "evaluate_noisy(noise, sampling=Sampling(...)) sample one at n = 2..12")
    N = branch.shape[0]
    pred = torch.empty(N, dtype=torch.float64, device=branch.device)
    shot_std = torch.empty(N, dtype=torch.float64, device=branch.device)
    chunk = max(1, WIDE_EXACT_STATE_BYTES >> (2 * n + 4))
    if chunk_rows is not None:
        chunk = max(1, min(chunk, int(chunk_rows)))
    nz = noise.params()
    for s in range(0, N, chunk):
        e = min(N, s + chunk)
        _lib.model_forward_noisy_exact_wide(desc, branch[s:e], None if trunk is None else trunk[s:e], flat, nz, ham_diag=ham_diag,
                                            out=pred[s:e], shot_std=shot_std[s:e])
    return pred.unsqueeze(-1), shot_std


def device_exact_noisy_predict(model, inputs, device_noise, chunk_rows=None):
    """
    exact_noisy_predict under a DeviceNoise for n = 2..9: (pred [N, 1], shot_std [N]).  n <= 6 is exact_noisy_predict itself
    (bitwise).  n = 7..9 runs qhea_model_forward_noisy_device_exact_wide: the per-wire channel sites of the device model on the
    tiles of wide_exact_noisy_predict, the density matrices of a chunk of rows in device memory, 4^n x 16 bytes per row.  Rows go
    in chunks of the largest count whose density matrices stay within 256 MiB (1024 / 256 / 64 rows at n = 7 / 8 / 9), and of no
    more than `chunk_rows` when given; the result is bitwise the same for any chunking.
    """
    if not isinstance(device_noise, DeviceNoise):
        raise ValueError(f"device_exact_noisy_predict takes a DeviceNoise (got {type(device_noise).__name__}); a NoiseModel goes to "
                         "wide_exact_noisy_predict, or through DeviceNoise.uniform")
    desc, flat, ham_diag, branch, trunk = _call_args(model, inputs, 'device_exact_noisy_predict')
    n = desc.n_qubits
    if n <= 6:
        return exact_noisy_predict(model, inputs, device_noise) if chunk_rows is None else \
            exact_noisy_predict(model, inputs, device_noise, chunk_rows=chunk_rows)
    if n >= 10:
        raise ValueError(f"device_exact_noisy_predict covers n = 2..9 (got n = {n}): a density matrix of 4^{n} elements per row "
                         "is not carried; device_noisy_predict estimates a DeviceNoise at n = 10..12 from quantum-jump "
                         "trajectories")
    N = branch.shape[0]
    pred = torch.empty(N, dtype=torch.float64, device=branch.device)
    shot_std = torch.empty(N, dtype=torch.float64, device=branch.device)
    chunk = max(1, WIDE_EXACT_STATE_BYTES >> (2 * n + 4))
    if chunk_rows is not None:
        chunk = max(1, min(chunk, int(chunk_rows)))
    nz = device_noise.params(n)
    for s in range(0, N, chunk):
        e = min(N, s + chunk)
        _lib.model_forward_noisy_device_exact_wide(desc, branch[s:e], None if trunk is None else trunk[s:e], flat, nz,
                                                   ham_diag=ham_diag, out=pred[s:e], shot_std=shot_std[s:e])
    return pred.unsqueeze(-1), shot_std


def amplification(model, noise):
    """
    log10 of the factor by which the gradient's inverse walk amplifies the traceless part of rho for this model's circuit
    under `noise`: (1 - 4 p1 / 3)^-L1 (1 - 16 p2 / 15)^-L2 over its L1 one-qubit and L2 CNOT noise locations.  The noise-aware
    training calls refuse values above 12 (and singular channels, inf); no device is needed.
    """
    if not hasattr(model, 'fused_desc'):
        raise TypeError("amplification takes a QuanONetPT or HEAQNNPT model")
    _uniform_only(noise, 'amplification', _GRADIENT_WHY)
    return _lib.model_exact_noisy_log10_amplification(model.fused_desc(), noise.params())


def exact_noisy_loss_and_grad(model, inputs, y, noise, inv_batch_total=None):
    """
    The MSE loss of the exact noisy prediction (exact_noisy_predict) and its exact gradient, as the flat [P + 2] tensor of
    qhea_model_loss_grad_noisy_exact: d/dparams of sum_b (pred_b - y_b)^2 * inv_batch_total in model.parameters() order, then
    sum (pred - y)^2 and sum y^2.  inv_batch_total defaults to 1 / rows (the mean); a shard of a larger batch passes the global
    value.  The gradient is computed by the adjoint walk through the density matrix: no sampling, n <= 6.
    """
    _uniform_only(noise, 'exact_noisy_loss_and_grad', _GRADIENT_WHY)
    desc, flat, ham_diag, branch, trunk = _call_args(model, inputs, 'exact_noisy_loss_and_grad')
    B = branch.shape[0]
    y = y.detach().to(torch.float64).reshape(-1).contiguous()
    grad = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=branch.device)
    if B == 0:
        return grad
    inv = 1.0 / B if inv_batch_total is None else float(inv_batch_total)
    return _lib.model_loss_grad_noisy_exact(desc, branch, trunk, y, flat, noise.params(), inv, grad, ham_diag=ham_diag)


def wide_exact_noisy_loss_and_grad(model, inputs, y, noise, inv_batch_total=None):
    """
    exact_noisy_loss_and_grad for n = 2..9: the flat [P + 2] tensor.  n <= 6 is exact_noisy_loss_and_grad itself (bitwise).
    n = 7..9 runs qhea_model_loss_grad_noisy_exact_wide: the same adjoint walk with rho and the observable of all rows in device
    memory, 2 x 4^n x 16 bytes per row, on the tiles of wide_exact_noisy_predict, whose pred this call's loss is built on bit
    for bit.  A NoiseModel only; the guard of exact_noisy_loss_and_grad (amplification(model, noise) <= 12) applies.
    """
    if isinstance(noise, DeviceNoise):
        raise ValueError("wide_exact_noisy_loss_and_grad takes a NoiseModel, not a DeviceNoise: the tiled reverse walk carries the "
                         "uniform channels only; device_noisy_loss_and_grad differentiates a DeviceNoise exactly at n <= 6 and "
                         "device_trajectory_loss_and_grad by quantum-jump trajectories at n = 7..12")
    if not hasattr(model, 'fused_desc'):
        raise TypeError("wide_exact_noisy_loss_and_grad takes a QuanONetPT or HEAQNNPT model")
    n = int(model.fused_desc().n_qubits)
    if n <= 6:
        return exact_noisy_loss_and_grad(model, inputs, y, noise, inv_batch_total)
    if n >= 10:
        raise ValueError(f"wide_exact_noisy_loss_and_grad covers n = 2..9 (got n = {n}): a density matrix of 4^{n} elements per "
                         "row is not carried; sampled_noisy_loss_and_grad differentiates the sampled loss at n = 10..12")
    desc, flat, ham_diag, branch, trunk = _call_args(model, inputs, 'wide_exact_noisy_loss_and_grad')
    B = branch.shape[0]
    y = y.detach().to(torch.float64).reshape(-1).contiguous()
    grad = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=branch.device)
    if B == 0:
        return grad
    inv = 1.0 / B if inv_batch_total is None else float(inv_batch_total)
    return _lib.model_loss_grad_noisy_exact_wide(desc, branch, trunk, y, flat, noise.params(), inv, grad, ham_diag=ham_diag)


def noisy_loss_and_grad(model, inputs, y, noise, inv_batch_total=None, row0=0):
    """
    The MSE loss of the SAMPLED noisy prediction -- noisy_predict(model, inputs, noise, row0=row0) in expectation mode, the mean
    of noise.trajectories runs on the stream keyed noise.seed -- and its gradient with that stream held fixed, as the flat
    [P + 2] tensor of qhea_model_loss_grad_noisy_wide (the layout of exact_noisy_loss_and_grad).  d pred / d params is an
    unbiased estimate of the exact noisy derivative; the loss also carries the trajectories' variance / T (the header states
    the estimator).  n = 7..9, where no density matrix fits in LDS; for n <= 6 exact_noisy_loss_and_grad is the call.
    """
    _uniform_only(noise, 'noisy_loss_and_grad',
                  "relaxation jumps depend on the state, so a sampled DeviceNoise has no fixed-stream gradient")
    if not hasattr(model, 'fused_desc'):
        raise TypeError("noisy_loss_and_grad takes a QuanONetPT or HEAQNNPT model")
    if noise.shots > 0:
        raise ValueError("noisy_loss_and_grad differentiates expectation mode (shots = 0); a sampled bitstring has no gradient")
    n = int(model.fused_desc().n_qubits)
    if n <= 6:
        raise ValueError(f"noisy_loss_and_grad covers n = 7..9 (got n = {n}); exact_noisy_loss_and_grad is the call for n <= 6")
    if n >= 10:
        raise ValueError(f"noisy_loss_and_grad covers n = 7..9 (got n = {n})")
    return _sampled_trajectory_call('noisy_loss_and_grad', model, inputs, y, noise, inv_batch_total, row0)


def _sampled_trajectory_call(who, model, inputs, y, noise, inv_batch_total, row0):
    desc, flat, ham_diag, branch, trunk = _call_args(model, inputs, who)
    B = branch.shape[0]
    y = y.detach().to(torch.float64).reshape(-1).contiguous()
    grad = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=branch.device)
    if B == 0:
        return grad
    inv = 1.0 / B if inv_batch_total is None else float(inv_batch_total)
    call, _ = _lib.sampled_grad_calls(desc.n_qubits)
    return call(desc, branch, trunk, y, flat, noise.params(), inv, grad, row0=int(row0), ham_diag=ham_diag)


def sampled_noisy_loss_and_grad(model, inputs, y, noise, inv_batch_total=None, row0=0):
    """
    noisy_loss_and_grad for every qubit count a sampled gradient exists for, n = 7..12: at n = 7..9 it IS noisy_loss_and_grad
    (qhea_model_loss_grad_noisy_wide, bitwise), at n = 10..12 the same quantity from qhea_model_loss_grad_noisy_lds (psi and
    lambda in LDS).  For n <= 6 exact_noisy_loss_and_grad is the call.
    """
    _uniform_only(noise, 'sampled_noisy_loss_and_grad',
                  "relaxation jumps depend on the state, so a sampled DeviceNoise has no fixed-stream gradient")
    if not hasattr(model, 'fused_desc'):
        raise TypeError("sampled_noisy_loss_and_grad takes a QuanONetPT or HEAQNNPT model")
    if noise.shots > 0:
        raise ValueError("sampled_noisy_loss_and_grad differentiates expectation mode (shots = 0); a sampled bitstring has no "
                         "gradient")
    n = int(model.fused_desc().n_qubits)
    if n <= 6:
        raise ValueError(f"sampled_noisy_loss_and_grad covers n = 7..12 (got n = {n}); exact_noisy_loss_and_grad is the call "
                         "for n <= 6")
    return _sampled_trajectory_call('sampled_noisy_loss_and_grad', model, inputs, y, noise, inv_batch_total, row0)


def _device_noise(noise, who):
    if not isinstance(noise, DeviceNoise):
        raise ValueError(f"{who} takes a DeviceNoise (got {type(noise).__name__}); a NoiseModel goes to its uniform "
                         "counterpart, or through DeviceNoise.uniform")


def device_amplification(model, noise):
    """
    log10 A_dev of this model's circuit under `noise` (a DeviceNoise): what the inverse walk of the device-noise gradient
    multiplies the traceless part of rho by, - sum log10 min(off, a) over the one-wire channel sites the circuit applies
    - sum log10 (1 - 16 p2[j] / 15) over its CNOT slots.  For DeviceNoise.uniform(nm) it is amplification(model, nm).  The
    training calls refuse values above 7 (and singular channels, inf): the bound is lower than the uniform walk's 12 because
    relaxation is not self-adjoint.  No device is needed.
    """
    if not hasattr(model, 'fused_desc'):
        raise TypeError("device_amplification takes a QuanONetPT or HEAQNNPT model")
    _device_noise(noise, 'device_amplification')
    desc = model.fused_desc()
    return _lib.model_device_noisy_log10_amplification(desc, noise.params(desc.n_qubits))


def device_layer_amplification(model, noise):
    """
    device_amplification of the largest single unit of this model's circuit (qhea_model_device_noisy_log10_layer_amplification):
    one sub-layer's channel sites and CNOT slots with the encoding sites in front of it.  It bounds
    device_noisy_loss_and_grad(states='stored') and the config key train_noise_states='stored', which replay rho from the
    state stored after every unit, the way device_amplification bounds the inverse walk (values above 7 and inf are refused).
    No device is needed.
    """
    if not hasattr(model, 'fused_desc'):
        raise TypeError("device_layer_amplification takes a QuanONetPT or HEAQNNPT model")
    _device_noise(noise, 'device_layer_amplification')
    desc = model.fused_desc()
    return _lib.model_device_noisy_log10_layer_amplification(desc, noise.params(desc.n_qubits))


NOISE_STATES = ('inverse', 'stored')


def device_noisy_loss_and_grad(model, inputs, y, noise, inv_batch_total=None, states='inverse'):
    """
    exact_noisy_loss_and_grad under a DeviceNoise: the MSE loss of exact_noisy_predict(model, inputs, noise) and its exact
    gradient, as the flat [P + 2] tensor of qhea_model_loss_grad_noisy_device_exact (same layout, same inv_batch_total).  The
    adjoint walk through the density matrix with the device's channel sites: no sampling, n <= 6.
    states='inverse' walks rho back through the inverse of every channel and is refused above device_amplification 7;
    states='stored' (qhea_model_loss_grad_noisy_device_exact_stored) replays rho from the state the forward sweep stored after
    every sub-layer, is bounded by device_layer_amplification instead, and takes units x rows x 16 x 4^n more bytes.
    """
    _device_noise(noise, 'device_noisy_loss_and_grad')
    if states not in NOISE_STATES:
        raise ValueError(f"device_noisy_loss_and_grad: states must be 'inverse' or 'stored' (got {states!r})")
    desc, flat, ham_diag, branch, trunk = _call_args(model, inputs, 'device_noisy_loss_and_grad')
    B = branch.shape[0]
    y = y.detach().to(torch.float64).reshape(-1).contiguous()
    grad = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=branch.device)
    if B == 0:
        return grad
    inv = 1.0 / B if inv_batch_total is None else float(inv_batch_total)
    call = _lib.model_loss_grad_noisy_device_exact_stored if states == 'stored' else _lib.model_loss_grad_noisy_device_exact
    return call(desc, branch, trunk, y, flat, noise.params(desc.n_qubits), inv, grad, ham_diag=ham_diag)


def device_exact_noisy_loss_and_grad(model, inputs, y, device_noise, inv_batch_total=None, states='inverse'):
    """
    device_noisy_loss_and_grad for n = 2..9: the flat [P + 2] tensor.  n <= 6 is device_noisy_loss_and_grad itself (inverse
    walk, bitwise).  n = 7..9 runs qhea_model_loss_grad_noisy_device_exact_wide: the same inverse walk with rho and the
    observable of all rows in device memory, 2 x 4^n x 16 bytes per row, on the tiles of device_exact_noisy_predict, whose pred
    this call's loss is built on bit for bit.  A DeviceNoise only; the guard of device_noisy_loss_and_grad
    (device_amplification(model, device_noise) <= 7) applies at every n.
    states='stored' replays rho from the state stored after every unit and is bounded by device_layer_amplification instead:
    at n <= 6 it is device_noisy_loss_and_grad(states='stored'), at n = 7..9 qhea_model_loss_grad_noisy_device_exact_wide_stored,
    whose forward sweep leaves every unit's rho in device memory (units x rows x 16 x 4^n more bytes) and whose pred is the
    inverse call's bit for bit.
    """
    if states not in NOISE_STATES:
        raise ValueError(f"device_exact_noisy_loss_and_grad: states must be 'inverse' or 'stored' (got {states!r})")
    if not isinstance(device_noise, DeviceNoise):
        raise ValueError(f"device_exact_noisy_loss_and_grad takes a DeviceNoise (got {type(device_noise).__name__}): a NoiseModel "
                         "goes to wide_exact_noisy_loss_and_grad (n = 2..9), or through DeviceNoise.uniform")
    if not hasattr(model, 'fused_desc'):
        raise TypeError("device_exact_noisy_loss_and_grad takes a QuanONetPT or HEAQNNPT model")
    n = int(model.fused_desc().n_qubits)
    if n <= 6:
        return device_noisy_loss_and_grad(model, inputs, y, device_noise, inv_batch_total, states)
    if n >= 10:
        raise ValueError(f"device_exact_noisy_loss_and_grad covers n = 2..9 (got n = {n}): a density matrix of 4^{n} elements "
                         "per row is not carried; device_trajectory_loss_and_grad differentiates the quantum-jump loss at "
                         "n = 7..12")
    desc, flat, ham_diag, branch, trunk = _call_args(model, inputs, 'device_exact_noisy_loss_and_grad')
    B = branch.shape[0]
    y = y.detach().to(torch.float64).reshape(-1).contiguous()
    grad = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=branch.device)
    if B == 0:
        return grad
    inv = 1.0 / B if inv_batch_total is None else float(inv_batch_total)
    call = _lib.model_loss_grad_noisy_device_exact_wide_stored if states == 'stored' else _lib.model_loss_grad_noisy_device_exact_wide
    return call(desc, branch, trunk, y, flat, device_noise.params(n), inv, grad, ham_diag=ham_diag)


def device_sampled_loss_and_grad(model, inputs, y, device_noise, sampling, inv_batch_total=None, row0=0):
    """
    The MSE loss of the quantum-jump estimate under a DeviceNoise -- device_noisy_predict(model, inputs, device_noise, sampling,
    row0=row0) in expectation mode -- and an unbiased gradient of it: (flat [P + 2] tensor of qhea_model_loss_grad_noisy_device,
    pred[B]).  Per trajectory the gradient of the UNNORMALISED numerator is taken with the fired jump pattern held fixed and
    divided by the final norm; neither the norm nor the jump decisions are differentiated (the two terms cancel: the header
    states the estimator).  The loss also carries the trajectories' variance / T.  n = 7..9, where no density matrix fits in
    LDS; for n <= 6 device_noisy_loss_and_grad is the exact call.
    """
    _device_noise(device_noise, 'device_sampled_loss_and_grad')
    if not isinstance(sampling, Sampling):
        raise ValueError(f"device_sampled_loss_and_grad takes a Sampling (got {type(sampling).__name__})")
    if not hasattr(model, 'fused_desc'):
        raise TypeError("device_sampled_loss_and_grad takes a QuanONetPT or HEAQNNPT model")
    if sampling.shots != 0:
        raise ValueError("device_sampled_loss_and_grad differentiates expectation mode (Sampling.shots = 0, trajectories = T); a "
                         "sampled bitstring has no gradient")
    n = int(model.fused_desc().n_qubits)
    if n <= 6:
        raise ValueError(f"device_sampled_loss_and_grad covers n = 7..9 (got n = {n}); device_noisy_loss_and_grad is the exact "
                         "call for n <= 6")
    if n >= 10:
        raise ValueError(f"device_sampled_loss_and_grad covers n = 7..9 (got n = {n}); device_trajectory_loss_and_grad is the "
                         "same call for n = 7..12")
    return _device_trajectory_call('device_sampled_loss_and_grad', model, inputs, y, device_noise, sampling, inv_batch_total, row0)


# The quantum-jump gradient kernels take psi back through a damping site that did not fire by K0^-1 = diag(1, 1 / sqrt(1 - gamma))
# and restore it only at sites that fired: a wire's run of unfired sites multiplies what rounding left in its |1> half by the
# product of those factors.  Largest site gamma at which the fp64 numpy form of that walk keeps 32 x its error below 2^-10 of the
# largest gradient entry on every case of tests/traj_precision_cases.py (10 and 20 blocks of LD 2 at n = 7 among them; the
# table is in DESIGN.md 7p).  At the next setting of that table (gamma >= 1 - 1.1e-4 on every wire) the walk is wrong in every
# digit.  Below the bound the error is heavy-tailed in the trajectory: this is the bound the table supports, not
# a guarantee.  The C calls (quanonet_amd._lib) refuse gamma = 1 only.
JUMP_GAMMA_MAX = 0.9998


def jump_gamma_max(device_noise, n):
    """(gamma, site name, wire) of the relaxation site of `device_noise` with the largest damping probability at n qubits
    (DeviceNoise.jump_tables; no device needed)"""
    gamma = np.asarray(device_noise.jump_tables(int(n)))[..., 0]
    site, wire = np.unravel_index(int(np.argmax(gamma)), gamma.shape)
    return float(gamma[site, wire]), _lib.SITE_NAMES[site], int(wire)


def check_jump_gradient_setting(device_noise, n, who):
    """ValueError for a setting whose largest site gamma is above JUMP_GAMMA_MAX (gamma = 1 keeps the message of
    qhea_device_noise_singular_site)"""
    gamma, site, wire = jump_gamma_max(device_noise, n)
    if gamma > JUMP_GAMMA_MAX and gamma < 1.0:
        raise ValueError(f"{who}: relaxation site {site} on wire {wire} has gamma = {gamma!r}, above {JUMP_GAMMA_MAX} "
                         "(quanonet_amd.noise.JUMP_GAMMA_MAX): the trajectory gradient walks psi back through unfired sites by "
                         "1 / sqrt(1 - gamma) and loses its digits there (DESIGN.md 7p)")


def _device_trajectory_call(who, model, inputs, y, device_noise, sampling, inv_batch_total, row0):
    check_jump_gradient_setting(device_noise, int(model.fused_desc().n_qubits), who)
    desc, flat, ham_diag, branch, trunk = _call_args(model, inputs, who)
    B = branch.shape[0]
    y = y.detach().to(torch.float64).reshape(-1).contiguous()
    grad = torch.zeros(flat.numel() + 2, dtype=torch.float64, device=branch.device)
    pred = torch.empty(B, dtype=torch.float64, device=branch.device)
    if B == 0:
        return grad, pred
    inv = 1.0 / B if inv_batch_total is None else float(inv_batch_total)
    call, _ = _lib.device_sampled_grad_calls(desc.n_qubits)
    call(desc, branch, trunk, y, flat, device_noise.params(desc.n_qubits), sampling.params(), inv, grad, row0=int(row0),
         ham_diag=ham_diag, pred=pred)
    return grad, pred


def device_trajectory_loss_and_grad(model, inputs, y, device_noise, sampling, inv_batch_total=None, row0=0):
    """
    device_sampled_loss_and_grad for every n a quantum-jump gradient exists for, n = 7..12: the MSE loss of the quantum-jump
    estimate under a DeviceNoise and the unbiased gradient of it (the same estimator and random stream at every n).  At
    n = 7..9 it is device_sampled_loss_and_grad, bitwise (qhea_model_loss_grad_noisy_device); at n = 10..12 psi and lambda live
    in LDS (qhea_model_loss_grad_noisy_device_lds) and pred is what device_noisy_predict returns there.  For n <= 6
    device_noisy_loss_and_grad is the exact call.
    """
    _device_noise(device_noise, 'device_trajectory_loss_and_grad')
    if not isinstance(sampling, Sampling):
        raise ValueError(f"device_trajectory_loss_and_grad takes a Sampling (got {type(sampling).__name__})")
    if not hasattr(model, 'fused_desc'):
        raise TypeError("device_trajectory_loss_and_grad takes a QuanONetPT or HEAQNNPT model")
    if sampling.shots != 0:
        raise ValueError("device_trajectory_loss_and_grad differentiates expectation mode (Sampling.shots = 0, trajectories = T); "
                         "a sampled bitstring has no gradient")
    n = int(model.fused_desc().n_qubits)
    if n <= 6:
        raise ValueError(f"device_trajectory_loss_and_grad covers n = 7..12 (got n = {n}); device_noisy_loss_and_grad is the "
                         "exact call for n <= 6")
    return _device_trajectory_call('device_trajectory_loss_and_grad', model, inputs, y, device_noise, sampling, inv_batch_total,
                                   row0)
