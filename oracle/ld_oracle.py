"""
ctypes loader for oracle/libhea_oracle_ld.so: oracle/hea_oracle.c built with long double as its scalar type
(-DQHEA_ORACLE_LONG_DOUBLE; at least 64 mantissa bits, asserted at compile time).  TEST INFRASTRUCTURE ONLY.

It is the reference the two fp64 oracles (c_oracle, hea_oracle) are themselves measured against.  Same call shape as
c_oracle, but every result v comes back as a pair of float64 arrays (hi, lo) with hi = (double)v and lo = (double)(v - hi),
so that Python needs neither np.longdouble nor ctypes.c_longdouble; the error of a float64 array ``got`` is
``err(got, pair)`` = (got - hi) - lo, evaluated in float64 (got - hi is exact whenever the two are within a factor 2).

Model level (quanonet_loss_and_grads / heaqnn_loss_and_grads): the frequency layers in * w + b on the tiled inputs, the
fixed-scale form, the bias, the residuals, the MSE and the chain rule into the frequency parameters are all done IN C, in
long double, behind the same compile-time switch (qhea_oracle_ld_model_loss_grad); Python only gathers the tiled input
columns (exact) and splits the result arrays by parameter name.
"""
import ctypes
import os
import subprocess
import numpy as np

from oracle import hea_oracle as O
from oracle.c_oracle import _cfg, _fit_columns, _p, _pauli

_HERE = os.path.dirname(os.path.abspath(__file__))
_NAME = 'libhea_oracle_ld.so'
_LIB = None


def build(force=False):
    so = os.path.join(_HERE, _NAME)
    src = os.path.join(_HERE, 'hea_oracle.c')
    if force or not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(['make', '-s', '-C', _HERE, _NAME])
    return so


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, _NAME)
        if not os.path.exists(so):
            so = build()
        _LIB = ctypes.CDLL(so)
        d = ctypes.POINTER(ctypes.c_double)
        i32 = ctypes.POINTER(ctypes.c_int32)
        cd, ci = ctypes.c_double, ctypes.c_int
        _LIB.qhea_oracle_ld_forward.restype = ci
        _LIB.qhea_oracle_ld_forward.argtypes = [ci, ci, i32, i32, ctypes.c_int64, d, d, d, d, cd, cd, d, ci, d, d, d, d]
        _LIB.qhea_oracle_ld_backward.restype = ci
        _LIB.qhea_oracle_ld_backward.argtypes = [ci, ci, i32, i32, ctypes.c_int64, d, d, cd, cd, d, ci, d] + [d] * 6
        _LIB.qhea_oracle_ld_model_loss_grad.restype = ci
        _LIB.qhea_oracle_ld_model_loss_grad.argtypes = ([ci, ci, i32, i32, ctypes.c_int64, d, d, d, d, cd, d, cd, cd, cd, d, ci]
                                                        + [d] * 10)
    return _LIB


def err(got, pair):
    """got - (hi + lo) in float64"""
    hi, lo = pair
    return (np.asarray(got, np.float64).reshape(hi.shape) - hi) - lo


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def hea_forward(num_qubits, block_configs, x, w, offset=0.0, coeff=1.0, ham_diag=None,
                return_state=False, ham_pauli='Z', x_lo=None, w_lo=None):
    """(out_hi, out_lo), and with return_state ((out_hi, out_lo), (state_hi, state_lo)); state [B, 2^n, 2].
    x_lo / w_lo: low parts of the angles, for angles that no float64 holds (the parameter-shift rule's theta + pi/2)."""
    x = _fit_columns(x, block_configs)
    w = _f64(w)
    x_lo = None if x_lo is None else _fit_columns(x_lo, block_configs)
    w_lo = _f64(w_lo)
    assert w_lo is None or w_lo.shape == w.shape
    diag = _f64(ham_diag)
    B = x.shape[0]
    enc, ld, pe, pl = _cfg(block_configs)
    out = (np.empty(B), np.empty(B))
    st = (np.empty((B, 1 << num_qubits, 2)), np.empty((B, 1 << num_qubits, 2))) if return_state else (None, None)
    rc = lib().qhea_oracle_ld_forward(num_qubits, len(block_configs), pe, pl, B, _p(x), _p(x_lo), _p(w), _p(w_lo),
                                      float(offset), float(coeff), _p(diag), _pauli(ham_pauli),
                                      _p(out[0]), _p(out[1]), _p(st[0]), _p(st[1]))
    if rc:
        raise ValueError(f"qhea_oracle_ld_forward failed ({rc})")
    return (out, st) if return_state else out


def hea_backward(num_qubits, block_configs, x, w, g, offset=0.0, coeff=1.0, ham_diag=None, ham_pauli='Z'):
    """((out_hi, out_lo), (gx_hi, gx_lo), (gw_hi, gw_lo)); x must have the circuit's own width"""
    x = _f64(x)
    assert x.shape[1] == sum(c[0] for c in block_configs)
    w = _f64(w)
    g = _f64(g).reshape(-1)
    diag = _f64(ham_diag)
    B = x.shape[0]
    enc, ld, pe, pl = _cfg(block_configs)
    out = (np.empty(B), np.empty(B))
    gx = (np.zeros_like(x), np.zeros_like(x))
    gw = (np.zeros_like(w), np.zeros_like(w))
    rc = lib().qhea_oracle_ld_backward(num_qubits, len(block_configs), pe, pl, B, _p(x), _p(w), float(offset), float(coeff),
                                       _p(diag), _pauli(ham_pauli), _p(g), _p(out[0]), _p(out[1]), _p(gx[0]), _p(gx[1]),
                                       _p(gw[0]), _p(gw[1]))
    if rc:
        raise ValueError(f"qhea_oracle_ld_backward failed ({rc})")
    return out, gx, gw


def _tiled(x_in, out_features):
    x_in = np.asarray(x_in, np.float64)
    return x_in[:, np.arange(out_features) % x_in.shape[1]]


def _freq(params, prefix, out_features, scale_coeff):
    """(fw[out], fb[out] or None, trainable) of one frequency layer, as hea_oracle._freq_encode reads them"""
    wkey, bkey = prefix + '.weights', prefix + '.bias'
    if wkey in params:
        fw = np.asarray(params[wkey], np.float64).reshape(-1)
        fb = np.asarray(params[bkey], np.float64).reshape(-1)
        assert fw.shape[0] == out_features and fb.shape[0] == out_features
        return fw, fb, True
    if scale_coeff is None:
        raise ValueError(f"no '{wkey}' in params: fixed-frequency mode needs scale_coeff")
    return np.full(out_features, float(scale_coeff)), None, False


def _model(num_qubits, cfgs, tin, fw, fb, w, bias, y, batch_total, ham_bound, ham_diag, ham_pauli):
    n = num_qubits
    tin, fw, w = _f64(tin), _f64(fw), _f64(w)
    y = _f64(y).reshape(-1)
    B, E = tin.shape
    assert E == sum(c[0] for c in cfgs) and fw.shape == (E,) and y.shape == (B,)
    fb = _f64(fb) if fb is not None else np.zeros(E)
    diag = _f64(ham_diag)
    off, co = O.ham_params(n, *ham_bound)
    enc, ld, pe, pl = _cfg(cfgs)
    pair = lambda shape: (np.zeros(shape), np.zeros(shape))
    sse, gbias, out, gw, gfw, gfb = np.zeros(2), np.zeros(2), pair(B), pair(w.shape), pair(E), pair(E)
    rc = lib().qhea_oracle_ld_model_loss_grad(n, len(cfgs), pe, pl, B, _p(tin), _p(fw), _p(fb), _p(w), float(bias), _p(y),
                                              float(batch_total), off, co, _p(diag), _pauli(ham_pauli), _p(sse),
                                              _p(out[0]), _p(out[1]), _p(gw[0]), _p(gw[1]), _p(gfw[0]), _p(gfw[1]),
                                              _p(gfb[0]), _p(gfb[1]), _p(gbias))
    if rc:
        raise ValueError(f"qhea_oracle_ld_model_loss_grad failed ({rc})")
    return sse, gbias, out, gw, gfw, gfb


def quanonet_loss_and_grads(params, branch, trunk, y, num_qubits, net_size, ham_bound=(-5.0, 5.0), batch_total=None,
                            ham_pauli='Z', scale_coeff=None, ham_diag=None):
    """hea_oracle.quanonet_loss_and_grads in long double (all of it in C, see the module docstring).  Returns
    (sse (hi, lo) -- the SUM of squared residuals, not the mean --, grads {name: (hi, lo)}, out (hi, lo))."""
    y = np.asarray(y, np.float64).reshape(-1)
    Bt = float(batch_total if batch_total is not None else y.shape[0])
    bd, bl, td, tl = net_size
    nt, nbr = td * num_qubits, bd * num_qubits
    tw, tb, t_train = _freq(params, 'trunk_freq', nt, scale_coeff)
    bw, bb, b_train = _freq(params, 'branch_freq', nbr, scale_coeff)
    tin = np.concatenate([_tiled(trunk, nt), _tiled(branch, nbr)], axis=1)            # trunk first
    fb = None if tb is None and bb is None else np.concatenate([tb if tb is not None else np.zeros(nt),
                                                                 bb if bb is not None else np.zeros(nbr)])
    cfgs = O.block_configs_quanonet(num_qubits, net_size)
    bias = float(np.asarray(params['bias']).reshape(-1)[0])
    sse, gbias, out, gw, gfw, gfb = _model(num_qubits, cfgs, tin, np.concatenate([tw, bw]), fb,
                                           params['quantum_layer.ansatz_weights'], bias, y, Bt, ham_bound, ham_diag, ham_pauli)
    grads = {'quantum_layer.ansatz_weights': gw, 'bias': (gbias[:1], gbias[1:])}
    if t_train:
        grads['trunk_freq.weights'] = (gfw[0][:nt], gfw[1][:nt])
        grads['trunk_freq.bias'] = (gfb[0][:nt], gfb[1][:nt])
    if b_train:
        grads['branch_freq.weights'] = (gfw[0][nt:], gfw[1][nt:])
        grads['branch_freq.bias'] = (gfb[0][nt:], gfb[1][nt:])
    return (sse[0], sse[1]), grads, out


def heaqnn_loss_and_grads(params, x_in, y, num_qubits, net_size, ham_bound=(-5.0, 5.0), batch_total=None,
                          ham_pauli='Z', scale_coeff=None, ham_diag=None):
    """hea_oracle.heaqnn_loss_and_grads in long double; same returns as quanonet_loss_and_grads here (no bias)."""
    y = np.asarray(y, np.float64).reshape(-1)
    Bt = float(batch_total if batch_total is not None else y.shape[0])
    E = net_size[0] * num_qubits
    fw, fb, train = _freq(params, 'freq', E, scale_coeff)
    cfgs = O.block_configs_heaqnn(num_qubits, net_size)
    sse, _, out, gw, gfw, gfb = _model(num_qubits, cfgs, _tiled(x_in, E), fw, fb, params['quantum_layer.ansatz_weights'],
                                       0.0, y, Bt, ham_bound, ham_diag, ham_pauli)
    grads = {'quantum_layer.ansatz_weights': gw}
    if train:
        grads['freq.weights'] = gfw
        grads['freq.bias'] = gfb
    return (sse[0], sse[1]), grads, out
