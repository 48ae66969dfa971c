"""
ctypes binding of the C ABI in include/quanonet_hea.h (libquanonet_hea.so, built in-tree by
``__graft_entry__.build()`` / ``quanonet_amd/csrc/Makefile``).

There is deliberately NO CPU fallback: if the shared library is missing, or a tensor is not on
a HIP device, the calls raise.  torch is used only for device memory and streams.
"""
import collections
import ctypes
import os

import torch

# Inter-process mapping of the data-parallel exchange buffers (qhea_dp_export / qhea_dp_import = hipIpcGetMemHandle /
# hipIpcOpenMemHandle) needs the dmabuf IPC mode on this driver stack: with the legacy mode hipIpcGetMemHandle fails with
# "invalid argument" and the trainer would fall back to the RCCL all-reduce.  The HSA runtime reads the variable when it
# is initialised, so the default is set here, at import, before this package makes its first HIP call; a process that had
# already initialised the GPU without it is told so by PeerExchange.create (its reason string).
IPC_ENV = 'HSA_ENABLE_IPC_MODE_LEGACY'
IPC_ENV_PRESET = os.environ.get(IPC_ENV)
IPC_ENV_SET_LATE = IPC_ENV_PRESET is None and torch.cuda.is_initialized()
os.environ.setdefault(IPC_ENV, '0')

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('QHEA_LIB') or os.path.join(_HERE, 'libquanonet_hea.so')   # QHEA_LIB: ablation/dev builds

EXPORTS = ['qhea_version', 'qhea_strerror', 'qhea_device_count', 'qhea_workspace_bytes',
           'qhea_forward', 'qhea_backward', 'qhea_model_param_count', 'qhea_model_workspace_bytes',
           'qhea_model_forward', 'qhea_model_forward_chunks', 'qhea_model_loss_grad', 'qhea_model_train_step', 'qhea_model_train_steps',
           'qhea_profile_next_circuit_kernel',
           'qhea_adam_step', 'qhea_set_backward_variant', 'qhea_check_status',
           'qhea_dp_buffer_bytes', 'qhea_dp_alloc', 'qhea_dp_free', 'qhea_dp_export', 'qhea_dp_import', 'qhea_dp_close',
           'qhea_dp_allreduce_adam', 'qhea_dp_status', 'qhea_model_dp_train_steps', 'qhea_clock_probe',
           'qhea_model_ensemble_workspace_bytes', 'qhea_model_ensemble_train_steps',
           'qhea_model_sweep_workspace_bytes', 'qhea_model_sweep_train_steps',
           'qhea_model_depth_sweep_workspace_bytes', 'qhea_model_depth_sweep_train_steps',
           'qhea_model_qubit_sweep_workspace_bytes', 'qhea_model_qubit_sweep_train_steps',
           'qhea_model_noisy_workspace_bytes', 'qhea_model_forward_noisy',
           'qhea_model_noisy_wide_workspace_bytes', 'qhea_model_forward_noisy_wide',
           'qhea_model_exact_noisy_workspace_bytes', 'qhea_model_forward_noisy_exact',
           'qhea_model_exact_noisy_wide_workspace_bytes', 'qhea_model_forward_noisy_exact_wide',
           'qhea_model_exact_noisy_grad_workspace_bytes', 'qhea_model_exact_noisy_log10_amplification',
           'qhea_model_loss_grad_noisy_exact', 'qhea_model_train_steps_noisy_exact',
           'qhea_model_exact_noisy_wide_grad_workspace_bytes', 'qhea_model_loss_grad_noisy_exact_wide',
           'qhea_model_train_steps_noisy_exact_wide',
           'qhea_device_noise_tables', 'qhea_model_forward_noisy_device_exact',
           'qhea_model_device_exact_noisy_wide_workspace_bytes', 'qhea_model_forward_noisy_device_exact_wide',
           'qhea_model_device_noisy_grad_workspace_bytes', 'qhea_model_device_noisy_log10_amplification',
           'qhea_model_loss_grad_noisy_device_exact', 'qhea_model_train_steps_noisy_device_exact',
           'qhea_device_noise_jump_tables', 'qhea_model_noisy_device_workspace_bytes', 'qhea_model_forward_noisy_device',
           'qhea_model_noisy_device_wide_workspace_bytes', 'qhea_model_forward_noisy_device_wide',
           'qhea_model_noisy_wide_grad_workspace_bytes', 'qhea_model_loss_grad_noisy_wide', 'qhea_model_train_steps_noisy_wide',
           'qhea_model_noisy_lds_grad_workspace_bytes', 'qhea_model_loss_grad_noisy_lds', 'qhea_model_train_steps_noisy_lds',
           'qhea_device_noise_singular_site', 'qhea_model_noisy_device_grad_workspace_bytes', 'qhea_model_loss_grad_noisy_device',
           'qhea_model_train_steps_noisy_device',
           'qhea_model_noisy_device_lds_grad_workspace_bytes', 'qhea_noisy_device_lds_grad_max_workgroups',
           'qhea_model_loss_grad_noisy_device_lds', 'qhea_model_train_steps_noisy_device_lds',
           'qhea_model_device_noisy_stored_grad_workspace_bytes', 'qhea_model_device_noisy_log10_layer_amplification',
           'qhea_model_loss_grad_noisy_device_exact_stored', 'qhea_model_train_steps_noisy_device_exact_stored',
           'qhea_model_device_noisy_wide_grad_workspace_bytes', 'qhea_model_loss_grad_noisy_device_exact_wide',
           'qhea_model_train_steps_noisy_device_exact_wide',
           'qhea_model_device_noisy_wide_stored_grad_workspace_bytes', 'qhea_model_loss_grad_noisy_device_exact_wide_stored',
           'qhea_model_train_steps_noisy_device_exact_wide_stored']


class ModelDesc(ctypes.Structure):
    """Mirror of `qhea_model_desc` (include/quanonet_hea.h)."""
    _fields_ = [('model', ctypes.c_int32), ('n_qubits', ctypes.c_int32), ('net', ctypes.c_int32 * 4),
                ('branch_in', ctypes.c_int32), ('trunk_in', ctypes.c_int32),
                ('trainable_freq', ctypes.c_int32), ('ham_pauli', ctypes.c_int32),
                ('scale_coeff', ctypes.c_double), ('ham_offset', ctypes.c_double), ('ham_coeff', ctypes.c_double)]


class MemberHParams(ctypes.Structure):
    """Mirror of `qhea_member_hparams` (include/quanonet_hea.h): one sweep member's read-out, fixed scale and learning rate."""
    _fields_ = [('scale_coeff', ctypes.c_double), ('ham_offset', ctypes.c_double), ('ham_coeff', ctypes.c_double),
                ('lr', ctypes.c_double), ('ham_pauli', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class NoiseParams(ctypes.Structure):
    """Mirror of `qhea_noise` (include/quanonet_hea.h): gate / readout error rates and the estimator of the noisy forward."""
    _fields_ = [('p1', ctypes.c_double), ('p2', ctypes.c_double), ('readout', ctypes.c_double), ('shots', ctypes.c_int64),
                ('trajectories', ctypes.c_int64), ('seed', ctypes.c_uint64)]


class DeviceNoiseParams(ctypes.Structure):
    """Mirror of `qhea_device_noise` (include/quanonet_hea.h): per-wire gate, readout and relaxation figures of a device and
    the layer durations.  The six arrays are host memory that the caller keeps alive for as long as the record is used."""
    _fields_ = [('n_wires', ctypes.c_int32), ('idle', ctypes.c_int32)] + \
               [(name, ctypes.POINTER(ctypes.c_double)) for name in ('p1', 'p2', 'readout01', 'readout10', 't1', 't2')] + \
               [('t_rx', ctypes.c_double), ('t_rot', ctypes.c_double), ('t_cx', ctypes.c_double)]


class SamplingParams(ctypes.Structure):
    """Mirror of `qhea_sampling` (include/quanonet_hea.h): the estimator of the device-noise trajectory call."""
    _fields_ = [('shots', ctypes.c_int64), ('trajectories', ctypes.c_int64), ('seed', ctypes.c_uint64)]


MODEL_QUANONET, MODEL_HEAQNN = 0, 1
MIN_LIB_VERSION = 670           # 0.6.7: + qhea_model_loss_grad_noisy_device_exact_wide_stored / ..._train_steps_... (stored states at n = 7..9)
BWD_VARIANTS = {'auto': 0, 'packed': 1, 'pair': 2, 'tri': 3, 'ztri': 4, 'zpacked': 5, 'ztri2': 6, 'zquad': 7, 'zsnap': 8}
PAULI = {'Z': 0, 'X': 1, 'Y': 2}


def pauli_code(p):
    """'Z'/'X'/'Y' (the reference's --ham_pauli choices, utils/common.py:81) or 0/1/2 -> QHEA_PAULI_*."""
    if isinstance(p, str):
        if p.upper() not in PAULI:
            raise ValueError(f"ham_pauli must be one of X, Y, Z (got {p!r})")
        return PAULI[p.upper()]
    if int(p) not in (0, 1, 2):
        raise ValueError(f"ham_pauli code must be 0, 1 or 2 (got {p!r})")
    return int(p)

_lib = None


class QheaError(RuntimeError):
    pass


def load():
    """Load libquanonet_hea.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QheaError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                        f"g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.qhea_version.restype = ctypes.c_int
    if lib.qhea_version() < MIN_LIB_VERSION:
        raise QheaError(f"{LIB_PATH} is version {lib.qhea_version()}, this binding needs >= {MIN_LIB_VERSION} "
                        f"(the model-sweep entry points): rebuild it")
    vp, dp = ctypes.c_void_p, ctypes.c_void_p
    i32p = ctypes.POINTER(ctypes.c_int32)
    lib.qhea_version.restype = ctypes.c_int
    lib.qhea_strerror.restype = ctypes.c_char_p
    lib.qhea_strerror.argtypes = [ctypes.c_int]
    lib.qhea_device_count.restype = ctypes.c_int
    lib.qhea_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, i32p, i32p, ctypes.c_int64]
    lib.qhea_forward.restype = ctypes.c_int
    lib.qhea_forward.argtypes = [ctypes.c_int, ctypes.c_int, i32p, i32p, ctypes.c_int64, dp, dp,
                                 ctypes.c_double, ctypes.c_double, dp, ctypes.c_int, dp, dp, vp, ctypes.c_size_t, vp]
    lib.qhea_backward.restype = ctypes.c_int
    lib.qhea_backward.argtypes = [ctypes.c_int, ctypes.c_int, i32p, i32p, ctypes.c_int64, dp, dp,
                                  ctypes.c_double, ctypes.c_double, dp, ctypes.c_int, dp, dp, dp, dp, dp,
                                  vp, ctypes.c_size_t, vp]
    lib.qhea_profile_next_circuit_kernel.restype = ctypes.c_int
    lib.qhea_profile_next_circuit_kernel.argtypes = [vp, vp]
    lib.qhea_set_backward_variant.restype = ctypes.c_int
    lib.qhea_set_backward_variant.argtypes = [ctypes.c_int]
    lib.qhea_check_status.restype = ctypes.c_int
    lib.qhea_check_status.argtypes = [vp, ctypes.c_size_t, vp]
    lib.qhea_adam_step.restype = ctypes.c_int
    lib.qhea_adam_step.argtypes = [ctypes.c_int64, dp, dp, dp, dp, ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                                   ctypes.c_double, ctypes.c_double, ctypes.c_double, vp]
    mdp = ctypes.POINTER(ModelDesc)
    i64p = ctypes.POINTER(ctypes.c_int64)
    f64p = ctypes.POINTER(ctypes.c_double)
    lib.qhea_model_forward_chunks.restype = ctypes.c_int
    lib.qhea_model_forward_chunks.argtypes = [mdp, ctypes.c_int64, i64p, dp, dp, dp, dp, dp, vp, ctypes.c_size_t, vp]
    lib.qhea_model_train_steps.restype = ctypes.c_int
    lib.qhea_model_train_steps.argtypes = [mdp, ctypes.c_int64, i64p, dp, dp, dp, dp, dp, f64p, dp, ctypes.c_int64, dp, dp,
                                           ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                           ctypes.c_double, ctypes.c_double, vp, ctypes.c_size_t, vp]
    vpp = ctypes.POINTER(ctypes.c_void_p)
    lib.qhea_dp_buffer_bytes.restype = ctypes.c_size_t
    lib.qhea_dp_buffer_bytes.argtypes = [ctypes.c_int64, ctypes.c_int]
    lib.qhea_dp_alloc.restype = ctypes.c_int
    lib.qhea_dp_alloc.argtypes = [ctypes.c_int64, ctypes.c_int, vpp]
    lib.qhea_dp_free.restype = ctypes.c_int
    lib.qhea_dp_free.argtypes = [vp]
    lib.qhea_dp_export.restype = ctypes.c_int
    lib.qhea_dp_export.argtypes = [vp, ctypes.c_char_p]
    lib.qhea_dp_import.restype = ctypes.c_int
    lib.qhea_dp_import.argtypes = [ctypes.c_char_p, vpp]
    lib.qhea_dp_close.restype = ctypes.c_int
    lib.qhea_dp_close.argtypes = [vp]
    lib.qhea_dp_allreduce_adam.restype = ctypes.c_int
    lib.qhea_dp_allreduce_adam.argtypes = [ctypes.c_int, ctypes.c_int, vpp, ctypes.c_int64, ctypes.c_int64, dp, dp,
                                           ctypes.c_int64, dp, dp, dp, ctypes.c_int64, ctypes.c_double,
                                           ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                           ctypes.c_double, vp]
    lib.qhea_dp_status.restype = ctypes.c_int
    lib.qhea_dp_status.argtypes = [vp, vp]
    lib.qhea_model_dp_train_steps.restype = ctypes.c_int
    lib.qhea_model_dp_train_steps.argtypes = [mdp, ctypes.c_int64, i64p, dp, dp, dp, dp, dp, f64p, dp, ctypes.c_int64, dp, dp,
                                              ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                              ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, vpp,
                                              ctypes.c_int64, ctypes.c_int64, ctypes.c_double, vp, ctypes.c_size_t, vp]
    lib.qhea_model_ensemble_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_ensemble_workspace_bytes.argtypes = [mdp, ctypes.c_int64, ctypes.c_int64]
    lib.qhea_model_ensemble_train_steps.restype = ctypes.c_int
    lib.qhea_model_ensemble_train_steps.argtypes = [mdp, ctypes.c_int64, ctypes.c_int64, i64p, dp, dp, dp, dp, dp, f64p, dp,
                                                    ctypes.c_int64, dp, dp, ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                                                    ctypes.c_double, ctypes.c_double, ctypes.c_double, vp, ctypes.c_size_t, vp]
    lib.qhea_model_sweep_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_sweep_workspace_bytes.argtypes = [mdp, ctypes.c_int64, ctypes.c_int64]
    lib.qhea_model_sweep_train_steps.restype = ctypes.c_int
    lib.qhea_model_sweep_train_steps.argtypes = [mdp, ctypes.c_int64, ctypes.POINTER(MemberHParams), dp, ctypes.c_int64, i64p,
                                                 dp, dp, dp, dp, f64p, dp, ctypes.c_int64, dp, dp, ctypes.c_int64,
                                                 ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, vp,
                                                 ctypes.c_size_t, vp]
    lib.qhea_model_depth_sweep_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_depth_sweep_workspace_bytes.argtypes = [mdp, ctypes.c_int64, ctypes.c_int64]
    lib.qhea_model_depth_sweep_train_steps.restype = ctypes.c_int
    lib.qhea_model_depth_sweep_train_steps.argtypes = [mdp, ctypes.c_int64, ctypes.POINTER(MemberHParams), dp, ctypes.c_int64,
                                                       i64p, dp, dp, dp, dp, f64p, dp, ctypes.c_int64, dp, dp, ctypes.c_int64,
                                                       ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, vp,
                                                       ctypes.c_size_t, vp]
    lib.qhea_model_qubit_sweep_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_qubit_sweep_workspace_bytes.argtypes = [mdp, ctypes.c_int64, ctypes.c_int64]
    lib.qhea_model_qubit_sweep_train_steps.restype = ctypes.c_int
    lib.qhea_model_qubit_sweep_train_steps.argtypes = lib.qhea_model_depth_sweep_train_steps.argtypes
    lib.qhea_clock_probe.restype = ctypes.c_int
    lib.qhea_clock_probe.argtypes = [ctypes.c_int, ctypes.c_int64, vp, vp]
    lib.qhea_model_param_count.restype = ctypes.c_int64
    lib.qhea_model_param_count.argtypes = [mdp]
    lib.qhea_model_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_workspace_bytes.argtypes = [mdp, ctypes.c_int64]
    lib.qhea_model_forward.restype = ctypes.c_int
    lib.qhea_model_forward.argtypes = [mdp, ctypes.c_int64, dp, dp, dp, dp, dp, vp, ctypes.c_size_t, vp]
    lib.qhea_model_loss_grad.restype = ctypes.c_int
    lib.qhea_model_loss_grad.argtypes = [mdp, ctypes.c_int64, dp, dp, dp, dp, dp, ctypes.c_double, dp, dp,
                                         vp, ctypes.c_size_t, vp]
    lib.qhea_model_train_step.restype = ctypes.c_int
    lib.qhea_model_train_step.argtypes = [mdp, ctypes.c_int64, dp, dp, dp, dp, dp, ctypes.c_double, dp, dp, dp, dp,
                                          ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                          ctypes.c_double, ctypes.c_double, vp, ctypes.c_size_t, vp]
    npp = ctypes.POINTER(NoiseParams)
    lib.qhea_model_noisy_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_noisy_workspace_bytes.argtypes = [mdp, ctypes.c_int64, npp]
    lib.qhea_model_forward_noisy.restype = ctypes.c_int
    lib.qhea_model_forward_noisy.argtypes = [mdp, ctypes.c_int64, ctypes.c_int64, dp, dp, dp, dp, npp, dp, dp, vp,
                                             ctypes.c_size_t, vp]
    lib.qhea_model_noisy_wide_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_noisy_wide_workspace_bytes.argtypes = lib.qhea_model_noisy_workspace_bytes.argtypes
    lib.qhea_model_forward_noisy_wide.restype = ctypes.c_int
    lib.qhea_model_forward_noisy_wide.argtypes = lib.qhea_model_forward_noisy.argtypes
    lib.qhea_model_exact_noisy_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_exact_noisy_workspace_bytes.argtypes = [mdp, ctypes.c_int64]
    lib.qhea_model_forward_noisy_exact.restype = ctypes.c_int
    lib.qhea_model_forward_noisy_exact.argtypes = [mdp, ctypes.c_int64, dp, dp, dp, dp, npp, dp, dp, vp, ctypes.c_size_t, vp]
    lib.qhea_model_exact_noisy_wide_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_exact_noisy_wide_workspace_bytes.argtypes = lib.qhea_model_exact_noisy_workspace_bytes.argtypes
    lib.qhea_model_forward_noisy_exact_wide.restype = ctypes.c_int
    lib.qhea_model_forward_noisy_exact_wide.argtypes = lib.qhea_model_forward_noisy_exact.argtypes
    lib.qhea_model_exact_noisy_grad_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_exact_noisy_grad_workspace_bytes.argtypes = [mdp, ctypes.c_int64]
    lib.qhea_model_exact_noisy_log10_amplification.restype = ctypes.c_double
    lib.qhea_model_exact_noisy_log10_amplification.argtypes = [mdp, npp]
    lib.qhea_model_loss_grad_noisy_exact.restype = ctypes.c_int
    lib.qhea_model_loss_grad_noisy_exact.argtypes = [mdp, ctypes.c_int64, dp, dp, dp, dp, dp, npp, ctypes.c_double, dp, dp, vp,
                                                     ctypes.c_size_t, vp]
    lib.qhea_model_train_steps_noisy_exact.restype = ctypes.c_int
    lib.qhea_model_train_steps_noisy_exact.argtypes = [mdp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), dp, dp, dp, dp, dp, npp,
                                                       ctypes.POINTER(ctypes.c_double), dp, ctypes.c_int64, dp, dp,
                                                       ctypes.c_int64] + [ctypes.c_double] * 5 + [vp, ctypes.c_size_t, vp]
    lib.qhea_model_exact_noisy_wide_grad_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_exact_noisy_wide_grad_workspace_bytes.argtypes = [mdp, ctypes.c_int64]
    lib.qhea_model_loss_grad_noisy_exact_wide.restype = ctypes.c_int
    lib.qhea_model_loss_grad_noisy_exact_wide.argtypes = lib.qhea_model_loss_grad_noisy_exact.argtypes
    lib.qhea_model_train_steps_noisy_exact_wide.restype = ctypes.c_int
    lib.qhea_model_train_steps_noisy_exact_wide.argtypes = lib.qhea_model_train_steps_noisy_exact.argtypes
    lib.qhea_model_noisy_wide_grad_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_noisy_wide_grad_workspace_bytes.argtypes = lib.qhea_model_noisy_workspace_bytes.argtypes
    lib.qhea_model_loss_grad_noisy_wide.restype = ctypes.c_int
    lib.qhea_model_loss_grad_noisy_wide.argtypes = [mdp, ctypes.c_int64] + lib.qhea_model_loss_grad_noisy_exact.argtypes[1:]
    lib.qhea_model_train_steps_noisy_wide.restype = ctypes.c_int
    lib.qhea_model_train_steps_noisy_wide.argtypes = lib.qhea_model_train_steps_noisy_exact.argtypes
    lib.qhea_model_noisy_lds_grad_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_noisy_lds_grad_workspace_bytes.argtypes = lib.qhea_model_noisy_wide_grad_workspace_bytes.argtypes
    lib.qhea_model_loss_grad_noisy_lds.restype = ctypes.c_int
    lib.qhea_model_loss_grad_noisy_lds.argtypes = lib.qhea_model_loss_grad_noisy_wide.argtypes
    lib.qhea_model_train_steps_noisy_lds.restype = ctypes.c_int
    lib.qhea_model_train_steps_noisy_lds.argtypes = lib.qhea_model_train_steps_noisy_wide.argtypes
    dnp = ctypes.POINTER(DeviceNoiseParams)
    lib.qhea_device_noise_tables.restype = ctypes.c_int
    lib.qhea_device_noise_tables.argtypes = [ctypes.c_int, dnp, f64p, f64p]
    lib.qhea_model_forward_noisy_device_exact.restype = ctypes.c_int
    lib.qhea_model_forward_noisy_device_exact.argtypes = [mdp, ctypes.c_int64, dp, dp, dp, dp, dnp, dp, dp, vp, ctypes.c_size_t, vp]
    lib.qhea_model_device_exact_noisy_wide_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_device_exact_noisy_wide_workspace_bytes.argtypes = lib.qhea_model_exact_noisy_workspace_bytes.argtypes
    lib.qhea_model_forward_noisy_device_exact_wide.restype = ctypes.c_int
    lib.qhea_model_forward_noisy_device_exact_wide.argtypes = lib.qhea_model_forward_noisy_device_exact.argtypes
    spp = ctypes.POINTER(SamplingParams)
    lib.qhea_device_noise_jump_tables.restype = ctypes.c_int
    lib.qhea_device_noise_jump_tables.argtypes = [ctypes.c_int, dnp, ctypes.POINTER(ctypes.c_double)]
    lib.qhea_model_noisy_device_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_noisy_device_workspace_bytes.argtypes = [mdp, ctypes.c_int64, spp]
    lib.qhea_model_forward_noisy_device.restype = ctypes.c_int
    lib.qhea_model_forward_noisy_device.argtypes = [mdp, ctypes.c_int64, ctypes.c_int64, dp, dp, dp, dp, dnp, spp, dp, dp, vp,
                                                    ctypes.c_size_t, vp]
    lib.qhea_model_noisy_device_wide_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_noisy_device_wide_workspace_bytes.argtypes = lib.qhea_model_noisy_device_workspace_bytes.argtypes
    lib.qhea_model_forward_noisy_device_wide.restype = ctypes.c_int
    lib.qhea_model_forward_noisy_device_wide.argtypes = lib.qhea_model_forward_noisy_device.argtypes
    lib.qhea_model_device_noisy_grad_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_device_noisy_grad_workspace_bytes.argtypes = [mdp, ctypes.c_int64]
    lib.qhea_model_device_noisy_log10_amplification.restype = ctypes.c_double
    lib.qhea_model_device_noisy_log10_amplification.argtypes = [mdp, dnp]
    lib.qhea_model_loss_grad_noisy_device_exact.restype = ctypes.c_int
    lib.qhea_model_loss_grad_noisy_device_exact.argtypes = [dnp if t is npp else t for t in lib.qhea_model_loss_grad_noisy_exact.argtypes]
    lib.qhea_model_device_noisy_stored_grad_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_device_noisy_stored_grad_workspace_bytes.argtypes = [mdp, ctypes.c_int64]
    lib.qhea_model_device_noisy_log10_layer_amplification.restype = ctypes.c_double
    lib.qhea_model_device_noisy_log10_layer_amplification.argtypes = [mdp, dnp]
    lib.qhea_model_loss_grad_noisy_device_exact_stored.restype = ctypes.c_int
    lib.qhea_model_loss_grad_noisy_device_exact_stored.argtypes = lib.qhea_model_loss_grad_noisy_device_exact.argtypes
    lib.qhea_model_train_steps_noisy_device_exact.restype = ctypes.c_int
    lib.qhea_model_train_steps_noisy_device_exact.argtypes = [dnp if t is npp else t
                                                              for t in lib.qhea_model_train_steps_noisy_exact.argtypes]
    lib.qhea_model_train_steps_noisy_device_exact_stored.restype = ctypes.c_int
    lib.qhea_model_train_steps_noisy_device_exact_stored.argtypes = lib.qhea_model_train_steps_noisy_device_exact.argtypes
    lib.qhea_model_device_noisy_wide_grad_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_device_noisy_wide_grad_workspace_bytes.argtypes = [mdp, ctypes.c_int64]
    lib.qhea_model_loss_grad_noisy_device_exact_wide.restype = ctypes.c_int
    lib.qhea_model_loss_grad_noisy_device_exact_wide.argtypes = lib.qhea_model_loss_grad_noisy_device_exact.argtypes
    lib.qhea_model_train_steps_noisy_device_exact_wide.restype = ctypes.c_int
    lib.qhea_model_train_steps_noisy_device_exact_wide.argtypes = lib.qhea_model_train_steps_noisy_device_exact.argtypes
    lib.qhea_model_device_noisy_wide_stored_grad_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_device_noisy_wide_stored_grad_workspace_bytes.argtypes = [mdp, ctypes.c_int64]
    lib.qhea_model_loss_grad_noisy_device_exact_wide_stored.restype = ctypes.c_int
    lib.qhea_model_loss_grad_noisy_device_exact_wide_stored.argtypes = lib.qhea_model_loss_grad_noisy_device_exact.argtypes
    lib.qhea_model_train_steps_noisy_device_exact_wide_stored.restype = ctypes.c_int
    lib.qhea_model_train_steps_noisy_device_exact_wide_stored.argtypes = lib.qhea_model_train_steps_noisy_device_exact.argtypes
    lib.qhea_device_noise_singular_site.restype = ctypes.c_int
    lib.qhea_device_noise_singular_site.argtypes = [ctypes.c_int, dnp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.qhea_model_noisy_device_grad_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_noisy_device_grad_workspace_bytes.argtypes = lib.qhea_model_noisy_device_workspace_bytes.argtypes
    lib.qhea_model_loss_grad_noisy_device.restype = ctypes.c_int
    lib.qhea_model_loss_grad_noisy_device.argtypes = [mdp, ctypes.c_int64, ctypes.c_int64, dp, dp, dp, dp, dp, dnp, spp, ctypes.c_double,
                                                      dp, dp, vp, ctypes.c_size_t, vp]
    lib.qhea_model_noisy_device_lds_grad_workspace_bytes.restype = ctypes.c_size_t
    lib.qhea_model_noisy_device_lds_grad_workspace_bytes.argtypes = lib.qhea_model_noisy_device_workspace_bytes.argtypes
    lib.qhea_noisy_device_lds_grad_max_workgroups.restype = ctypes.c_int
    lib.qhea_noisy_device_lds_grad_max_workgroups.argtypes = [ctypes.c_int]
    lib.qhea_model_train_steps_noisy_device.restype = ctypes.c_int
    lib.qhea_model_train_steps_noisy_device.argtypes = [mdp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), dp, dp, dp, dp, dp, dnp,
                                                        spp, ctypes.POINTER(ctypes.c_double), dp, ctypes.c_int64, dp, dp,
                                                        ctypes.c_int64] + [ctypes.c_double] * 5 + [vp, ctypes.c_size_t, vp]
    lib.qhea_model_loss_grad_noisy_device_lds.restype = ctypes.c_int
    lib.qhea_model_loss_grad_noisy_device_lds.argtypes = lib.qhea_model_loss_grad_noisy_device.argtypes
    lib.qhea_model_train_steps_noisy_device_lds.restype = ctypes.c_int
    lib.qhea_model_train_steps_noisy_device_lds.argtypes = lib.qhea_model_train_steps_noisy_device.argtypes
    _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        raise QheaError(f"{what} failed: {load().qhea_strerror(rc).decode()} ({rc})")


class CircuitShape:
    """Host-side description of the block list; owns the int32 arrays handed to the C ABI."""

    def __init__(self, num_qubits, block_configs):
        self.n = int(num_qubits)
        self.block_configs = [(int(a), int(b)) for a, b in block_configs]
        nb = len(self.block_configs)
        self._enc = (ctypes.c_int32 * max(nb, 1))(*[c[0] for c in self.block_configs])
        self._ld = (ctypes.c_int32 * max(nb, 1))(*[c[1] for c in self.block_configs])
        self.nb = nb
        self.E = sum(c[0] for c in self.block_configs)
        self.blk = sum(c[1] for c in self.block_configs)

    def workspace_bytes(self, batch):
        return int(load().qhea_workspace_bytes(self.n, self.nb, self._enc, self._ld, int(batch)))


def _dev_f64(t, name, shape=None):
    if t is None:
        return None
    if not t.is_cuda:
        raise QheaError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
    if t.dtype != torch.float64 or not t.is_contiguous():
        raise QheaError(f"{name} must be a contiguous float64 tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise QheaError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_workspaces = {}


def _model_ws(desc, rows, device):
    """Workspace for a model-level call on `rows` rows; the size query runs with `device` current (the layout follows that
    device's SIMD count)."""
    with torch.cuda.device(device):
        nbytes = int(load().qhea_model_workspace_bytes(ctypes.byref(desc), int(rows)))
    return _workspace(device, nbytes)


def _sized_ws(device, size_fn, *args):
    """The workspace a size function asks for, queried with `device` current; None where it answers 0 (the call that follows
    then reports what is wrong with its arguments)."""
    with torch.cuda.device(device):
        nbytes = int(size_fn(*args))
    return _workspace(device, nbytes) if nbytes else None


def _workspace(device, nbytes):
    """Grow-only per-device scratch tensor (caller-owned from the C ABI's point of view)."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            check_status(device)                    # the old buffer's status word must not be lost when growing
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def set_backward_variant(name):
    """'auto' | 'packed' | 'pair' | 'tri' | 'ztri': qhea_set_backward_variant (n <= 5 kernels; tests and sweeps)."""
    if name not in BWD_VARIANTS:
        raise ValueError(f"backward variant must be one of {sorted(BWD_VARIANTS)} (got {name!r})")
    _check(load().qhea_set_backward_variant(BWD_VARIANTS[name]), 'qhea_set_backward_variant')


def check_status(device):
    """
    qhea_check_status on this device's workspace: waits for the current stream and raises QheaError if a pipelined
    backward kernel reported a hand-off overrun since the last check (the gradients of that call were NaN-poisoned
    and its fused Adam update skipped).  No-op for a device that has not run anything yet.
    """
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    ws = _workspaces.get(key)
    if ws is None:
        return
    with torch.cuda.device(device):
        rc = load().qhea_check_status(_ptr(ws), ws.numel(), _stream(device))
    _check(rc, 'qhea_check_status')


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def hea_forward(shape, x, w, ham_offset, ham_coeff, ham_diag=None, return_state=False, ham_pauli=0):
    """out[B] (and optionally the final state [B,2^n,2]) on x.device.  No bias."""
    lib = load()
    B = x.shape[0]
    _dev_f64(x, 'x', (B, shape.E))
    _dev_f64(w, 'w', (shape.blk, 3, shape.n))
    _dev_f64(ham_diag, 'ham_diag', (1 << shape.n,))
    out = torch.empty(B, dtype=torch.float64, device=x.device)
    state = torch.empty((B, 1 << shape.n, 2), dtype=torch.float64, device=x.device) if return_state else None
    with torch.cuda.device(x.device):                 # the layout follows the current device's SIMD count
        nbytes = shape.workspace_bytes(B)
    ws = _workspace(x.device, nbytes)
    with torch.cuda.device(x.device):
        rc = lib.qhea_forward(shape.n, shape.nb, shape._enc, shape._ld, B, _ptr(x), _ptr(w),
                              float(ham_offset), float(ham_coeff), _ptr(ham_diag), pauli_code(ham_pauli),
                              _ptr(out), _ptr(state),
                              _ptr(ws), ws.numel(), _stream(x.device))
    _check(rc, 'qhea_forward')
    return (out, state) if return_state else out


def hea_backward(shape, x, w, g, ham_offset, ham_coeff, ham_diag=None, state=None, want_out=False, ham_pauli=0):
    """(grad_x[B,E], grad_w[blk,3,n][, out[B]]) for upstream g[B]."""
    lib = load()
    B = x.shape[0]
    _dev_f64(x, 'x', (B, shape.E))
    _dev_f64(w, 'w', (shape.blk, 3, shape.n))
    _dev_f64(g, 'g', (B,))
    _dev_f64(ham_diag, 'ham_diag', (1 << shape.n,))
    _dev_f64(state, 'state', (B, 1 << shape.n, 2))
    grad_x = torch.empty_like(x)
    grad_w = torch.empty_like(w)
    out = torch.empty(B, dtype=torch.float64, device=x.device) if want_out else None
    with torch.cuda.device(x.device):                 # the layout follows the current device's SIMD count
        nbytes = shape.workspace_bytes(B)
    ws = _workspace(x.device, nbytes)
    with torch.cuda.device(x.device):
        rc = lib.qhea_backward(shape.n, shape.nb, shape._enc, shape._ld, B, _ptr(x), _ptr(w),
                               float(ham_offset), float(ham_coeff), _ptr(ham_diag), pauli_code(ham_pauli),
                               _ptr(g), _ptr(state),
                               _ptr(out), _ptr(grad_x), _ptr(grad_w), _ptr(ws), ws.numel(),
                               _stream(x.device))
    _check(rc, 'qhea_backward')
    return (grad_x, grad_w, out) if want_out else (grad_x, grad_w)


# ---------------------------------------------------------------------------------------------------
# model-level (fused) calls
# ---------------------------------------------------------------------------------------------------
def make_model_desc(model, n_qubits, net_size, branch_in, trunk_in, trainable_freq, scale_coeff,
                    ham_offset, ham_coeff, ham_pauli=0):
    net = list(net_size) + [0] * (4 - len(net_size))
    d = ModelDesc(int(model), int(n_qubits), (ctypes.c_int32 * 4)(*[int(v) for v in net[:4]]), int(branch_in),
                  int(trunk_in), 1 if trainable_freq else 0, pauli_code(ham_pauli), float(scale_coeff), float(ham_offset),
                  float(ham_coeff))
    return d


def _model_inputs(desc, branch, trunk, params, ham_diag):
    """What every model-level call checks of its inputs; returns the row count."""
    B = branch.shape[0]
    _dev_f64(branch, 'branch', (B, desc.branch_in))
    if desc.model == MODEL_QUANONET:
        _dev_f64(trunk, 'trunk', (B, desc.trunk_in))
    _dev_f64(params, 'params')
    _dev_f64(ham_diag, 'ham_diag', (1 << desc.n_qubits,))
    return B


def model_param_count(desc):
    n = int(load().qhea_model_param_count(ctypes.byref(desc)))
    if n < 0:
        _check(n, 'qhea_model_param_count')
    return n


def model_forward(desc, branch, trunk, params, ham_diag=None, out=None):
    lib = load()
    B = _model_inputs(desc, branch, trunk, params, ham_diag)
    pred = out if out is not None else torch.empty(B, dtype=torch.float64, device=branch.device)
    ws = _model_ws(desc, B, branch.device)
    with torch.cuda.device(branch.device):
        rc = lib.qhea_model_forward(ctypes.byref(desc), B, _ptr(branch), _ptr(trunk), _ptr(params), _ptr(ham_diag),
                                    _ptr(pred), _ptr(ws), ws.numel(), _stream(branch.device))
    _check(rc, 'qhea_model_forward')
    return pred


def model_forward_chunks(desc, branch, trunk, params, chunk, ham_diag=None, out=None):
    """model_forward over all rows in chunks of `chunk` rows from ONE host call: one record preparation for all equal-sized
    chunks (qhea_model_forward_chunks); bitwise the chunk-by-chunk calls."""
    lib = load()
    N = _model_inputs(desc, branch, trunk, params, ham_diag)
    pred = out if out is not None else torch.empty(N, dtype=torch.float64, device=branch.device)
    if N == 0:
        return pred
    chunk = max(1, int(chunk))
    bounds = list(range(0, N, chunk)) + [N]
    ws = _model_ws(desc, min(chunk, N), branch.device)
    rb = (ctypes.c_int64 * len(bounds))(*bounds)
    with torch.cuda.device(branch.device):
        rc = lib.qhea_model_forward_chunks(ctypes.byref(desc), len(bounds) - 1, rb, _ptr(branch), _ptr(trunk), _ptr(params),
                                           _ptr(ham_diag), _ptr(pred), _ptr(ws), ws.numel(), _stream(branch.device))
    _check(rc, 'qhea_model_forward_chunks')
    return pred


def model_loss_grad(desc, branch, trunk, y, params, inv_batch_total, grad, ham_diag=None, pred=None):
    """Fills grad[P+2] = [d loss/d params | sse | sum y^2] for this shard; returns grad."""
    lib = load()
    B = _model_inputs(desc, branch, trunk, params, ham_diag)
    _dev_f64(y, 'y')
    if y.numel() != B:
        raise QheaError(f"y has {y.numel()} elements, expected {B}")
    _dev_f64(grad, 'grad')
    _dev_f64(pred, 'pred', (B,))
    ws = _model_ws(desc, B, branch.device)
    with torch.cuda.device(branch.device):
        rc = lib.qhea_model_loss_grad(ctypes.byref(desc), B, _ptr(branch), _ptr(trunk), _ptr(y), _ptr(params),
                                      _ptr(ham_diag), float(inv_batch_total), _ptr(grad), _ptr(pred),
                                      _ptr(ws), ws.numel(), _stream(branch.device))
    _check(rc, 'qhea_model_loss_grad')
    return grad


def model_train_step(desc, branch, trunk, y, params, inv_batch_total, grad, exp_avg, exp_avg_sq, step, lr, beta1,
                     beta2, eps, weight_decay, ham_diag=None, pred=None):
    """Single-device step: loss + gradients + Adam update of `params` in three launches; returns grad."""
    lib = load()
    B = _model_inputs(desc, branch, trunk, params, ham_diag)
    _dev_f64(y, 'y')
    if y.numel() != B:
        raise QheaError(f"y has {y.numel()} elements, expected {B}")
    for t, nm in ((grad, 'grad'), (exp_avg, 'exp_avg'), (exp_avg_sq, 'exp_avg_sq')):
        _dev_f64(t, nm)
    if not (exp_avg.numel() == exp_avg_sq.numel() == params.numel() and grad.numel() == params.numel() + 2):
        raise QheaError("model_train_step: flat vectors have inconsistent lengths")
    _dev_f64(pred, 'pred', (B,))
    ws = _model_ws(desc, B, branch.device)
    with torch.cuda.device(branch.device):
        rc = lib.qhea_model_train_step(ctypes.byref(desc), B, _ptr(branch), _ptr(trunk), _ptr(y), _ptr(params),
                                       _ptr(ham_diag), float(inv_batch_total), _ptr(grad), _ptr(pred),
                                       _ptr(exp_avg), _ptr(exp_avg_sq), int(step), float(lr), float(beta1),
                                       float(beta2), float(eps), float(weight_decay), _ptr(ws), ws.numel(),
                                       _stream(branch.device))
    _check(rc, 'qhea_model_train_step')
    return grad


def _schedule(bounds, global_batches):
    """(n_steps, row_begin, inv_batch_total, largest batch) of a training schedule: the two arrays as the C ABI takes them."""
    n_steps = len(bounds) - 1
    rb = (ctypes.c_int64 * (n_steps + 1))(*[int(b) for b in bounds])
    ib = (ctypes.c_double * n_steps)(*[1.0 / float(g) for g in global_batches])
    return n_steps, rb, ib, max(bounds[i + 1] - bounds[i] for i in range(n_steps))


def _flat_train_schedule(who, desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq, ham_diag):
    """The argument checks of the single-model schedule calls (who: the public function, for the messages); their _schedule."""
    n_steps = len(bounds) - 1
    N = branch.shape[0]
    _dev_f64(branch, 'branch', (N, desc.branch_in))
    if desc.model == MODEL_QUANONET:
        _dev_f64(trunk, 'trunk', (N, desc.trunk_in))
    _dev_f64(y, 'y')
    for t, nm in ((params, 'params'), (rows, 'rows'), (exp_avg, 'exp_avg'), (exp_avg_sq, 'exp_avg_sq')):
        _dev_f64(t, nm)
    P = params.numel()
    if y.numel() != N or bounds[-1] > N or len(global_batches) != n_steps:
        raise QheaError(f"{who}: row bounds do not match the arrays")
    if rows.dim() != 2 or rows.shape[0] < n_steps or rows.shape[1] < P + 2 or exp_avg.numel() != P or exp_avg_sq.numel() != P:
        raise QheaError(f"{who}: flat vectors have inconsistent lengths")
    _dev_f64(ham_diag, 'ham_diag', (1 << desc.n_qubits,))
    return _schedule(bounds, global_batches)


def model_train_steps(desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq, first_step, lr,
                      beta1, beta2, eps, weight_decay, ham_diag=None):
    """
    One epoch's inner loop in one host call (qhea_model_train_steps): step i trains on rows bounds[i]:bounds[i+1] of the
    contiguous branch / trunk / y with residual weight 1 / global_batches[i] and leaves [grads | sse | sum y^2] in rows[i].
    """
    lib = load()
    if len(bounds) - 1 <= 0:
        return rows
    n_steps, rb, ib, biggest = _flat_train_schedule('model_train_steps', desc, bounds, global_batches, branch, trunk, y, params,
                                                    rows, exp_avg, exp_avg_sq, ham_diag)
    ws = _model_ws(desc, biggest, branch.device)
    with torch.cuda.device(branch.device):
        rc = lib.qhea_model_train_steps(ctypes.byref(desc), n_steps, rb, _ptr(branch), _ptr(trunk), _ptr(y), _ptr(params),
                                        _ptr(ham_diag), ib, _ptr(rows), int(rows.stride(0)), _ptr(exp_avg),
                                        _ptr(exp_avg_sq), int(first_step), float(lr), float(beta1), float(beta2),
                                        float(eps), float(weight_decay), _ptr(ws), ws.numel(), _stream(branch.device))
    _check(rc, 'qhea_model_train_steps')
    return rows


def _desc_array(descs):
    descs = list(descs)
    return (ModelDesc * max(1, len(descs)))(*descs), len(descs)


def _member_train_steps(who, descs, members, lr, ws_bytes, zero_msg, diag_qubits, bounds, global_batches, branch, trunk, y,
                        params, rows, exp_avg, exp_avg_sq, first_step, beta1, beta2, eps, weight_decay, ham_diag):
    """
    What model_ensemble / sweep / depth_sweep / qubit_sweep_train_steps share: the checks of the [R, N, ...] inputs, the [R, P]
    state and the [R, n_steps, >= P+2] rows, the workspace, the marshalling and the call of qhea_<who>.  who: the public
    function (for the messages).  descs: [desc], or -- zero_msg given -- the R members' descriptors, P then being the largest
    member's parameter count and zero_msg the message for descriptors the library cannot take as one sweep.  members: the R
    MemberHParams, or None for an ensemble (one lr, one shared ham_diag).  ws_bytes(R, batch): the workspace size query;
    diag_qubits(descs): the qubit count that sizes a ham_diag row.
    """
    lib = load()
    n_steps = len(bounds) - 1
    if n_steps <= 0:
        return rows
    if branch.dim() != 3:
        raise QheaError(f"{who}: branch must be [n_models, rows, branch_in]")
    R, N = branch.shape[0], branch.shape[1]
    per_member = zero_msg is not None
    if members is not None and (len(members) != R or (per_member and len(descs) != R)):
        n_descs = f"{len(descs)} descriptors / " if per_member else ""
        raise QheaError(f"{who}: {n_descs}{len(members)} member records for {R} members")
    d0 = descs[0]
    _dev_f64(branch, 'branch', (R, N, d0.branch_in))
    if d0.model == MODEL_QUANONET:
        _dev_f64(trunk, 'trunk', (R, N, d0.trunk_in))
    _dev_f64(y, 'y')
    if tuple(y.shape) not in ((R, N), (R, N, 1)):
        raise QheaError(f"y has shape {tuple(y.shape)}, expected ({R}, {N})")
    for t, nm in ((params, 'params'), (rows, 'rows'), (exp_avg, 'exp_avg'), (exp_avg_sq, 'exp_avg_sq')):
        _dev_f64(t, nm)
    if per_member:
        P = depth_sweep_pmax(descs)
        p_name, p_shape = 'Pmax', f'Pmax = {P}'
    else:
        P = params.shape[-1] if params.dim() == 2 else -1
        p_name, p_shape = 'P', 'P'
    if tuple(params.shape) != (R, P) or tuple(exp_avg.shape) != (R, P) or tuple(exp_avg_sq.shape) != (R, P):
        raise QheaError(f"{who}: params / exp_avg / exp_avg_sq must be [n_models, {p_shape}]")
    if rows.dim() != 3 or rows.shape[0] != R or rows.shape[1] != n_steps or rows.shape[2] < P + 2:
        raise QheaError(f"{who}: rows must be [n_models, n_steps, >= {p_name}+2]")
    if bounds[0] < 0 or bounds[-1] != N or len(global_batches) != n_steps:
        raise QheaError(f"{who}: row bounds do not match the arrays")
    _dev_f64(ham_diag, 'ham_diag', (() if members is None else (R,)) + (1 << diag_qubits(descs),))
    with torch.cuda.device(branch.device):
        nbytes = max(ws_bytes(R, b) for b in sorted({bounds[i + 1] - bounds[i] for i in range(n_steps)}))
    if per_member and nbytes == 0:
        raise QheaError(f"{who}: {zero_msg}")
    ws = _workspace(branch.device, nbytes)
    n_steps, rb, ib, _ = _schedule(bounds, global_batches)
    head = (_desc_array(descs)[0], R)
    data = (_ptr(branch), _ptr(trunk), _ptr(y), _ptr(params))
    state = (ib, _ptr(rows), int(rows.stride(1)), _ptr(exp_avg), _ptr(exp_avg_sq), int(first_step))
    rest = (float(beta1), float(beta2), float(eps), float(weight_decay), _ptr(ws), ws.numel(), _stream(branch.device))
    if members is None:
        args = head + (n_steps, rb) + data + (_ptr(ham_diag),) + state + (float(lr),) + rest
    else:
        args = head + ((MemberHParams * R)(*members), _ptr(ham_diag), n_steps, rb) + data + state + rest
    with torch.cuda.device(branch.device):
        rc = getattr(lib, 'qhea_' + who)(*args)
    _check(rc, 'qhea_' + who)
    return rows


def _same_qubits(descs):
    return descs[0].n_qubits


def model_ensemble_workspace_bytes(desc, n_models, batch):
    """qhea_model_ensemble_workspace_bytes (current device's layout rules)."""
    return int(load().qhea_model_ensemble_workspace_bytes(ctypes.byref(desc), int(n_models), int(batch)))


def model_ensemble_train_steps(desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq, first_step,
                               lr, beta1, beta2, eps, weight_decay, ham_diag=None):
    """
    model_train_steps for R independent models of one descriptor, each step of all R members as one launch per kernel
    (qhea_model_ensemble_train_steps).  branch / trunk: [R, N, width], y: [R, N], params / exp_avg / exp_avg_sq: [R, P],
    rows: [R, n_steps, >= P+2]; every member follows the same schedule (bounds, global_batches).  Bitwise what
    model_train_steps gives for each member alone under the backward variant the ensemble chose.
    """
    return _member_train_steps('model_ensemble_train_steps', [desc], None, lr,
                               lambda R, b: model_ensemble_workspace_bytes(desc, R, b), None, _same_qubits,
                               bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq, first_step,
                               beta1, beta2, eps, weight_decay, ham_diag)


def member_hparams(scale_coeff, ham_offset, ham_coeff, lr, ham_pauli=0):
    """One sweep member's MemberHParams (ham_pauli: 'Z' / 'X' / 'Y' or QHEA_PAULI_*)."""
    return MemberHParams(float(scale_coeff), float(ham_offset), float(ham_coeff), float(lr), pauli_code(ham_pauli), 0)


def model_sweep_workspace_bytes(desc, n_models, batch):
    """qhea_model_sweep_workspace_bytes (current device's layout rules)."""
    return int(load().qhea_model_sweep_workspace_bytes(ctypes.byref(desc), int(n_models), int(batch)))


def model_sweep_train_steps(desc, members, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq,
                            first_step, beta1, beta2, eps, weight_decay, ham_diag=None):
    """
    model_ensemble_train_steps for members that also differ in read-out, fixed scale and learning rate
    (qhea_model_sweep_train_steps): `members` is a sequence of R MemberHParams (member_hparams), ham_diag None or [R, 2^n].
    desc fixes the shape only.  Bitwise what model_train_steps gives for each member alone, with that member's descriptor,
    learning rate and ham_diag row, under the backward variant the sweep chose.
    """
    return _member_train_steps('model_sweep_train_steps', [desc], members, None,
                               lambda R, b: model_sweep_workspace_bytes(desc, R, b), None, _same_qubits,
                               bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq, first_step,
                               beta1, beta2, eps, weight_decay, ham_diag)


def model_depth_sweep_workspace_bytes(descs, batch):
    """qhea_model_depth_sweep_workspace_bytes for the members' descriptors (current device's layout rules); 0 if they cannot
    train as one depth sweep."""
    arr, R = _desc_array(descs)
    return int(load().qhea_model_depth_sweep_workspace_bytes(arr, R, int(batch)))


def depth_sweep_pmax(descs):
    """Row length of a depth or qubit sweep's parameter / moment arrays: the largest member's model_param_count."""
    return max(model_param_count(d) for d in descs)


qubit_sweep_pmax = depth_sweep_pmax


def model_depth_sweep_train_steps(descs, members, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq,
                                  first_step, beta1, beta2, eps, weight_decay, ham_diag=None):
    """
    model_sweep_train_steps for members whose circuits also differ in depth (qhea_model_depth_sweep_train_steps): descs is the
    list of R member descriptors (equal but for the depth entries of net), members R MemberHParams.  params / exp_avg /
    exp_avg_sq: [R, Pmax], member m's vector at the front of row m; rows: [R, n_steps, >= Pmax + 2], member m's row holds its P_m
    gradients, then sse and sum y^2.  Member m gets bitwise what model_train_steps gives for it alone under the packed backward
    variant (n <= 9).
    """
    return _member_train_steps('model_depth_sweep_train_steps', descs, members, None,
                               lambda R, b: model_depth_sweep_workspace_bytes(descs, b),
                               "the descriptors differ in more than their depths", _same_qubits,
                               bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq, first_step,
                               beta1, beta2, eps, weight_decay, ham_diag)


def model_qubit_sweep_workspace_bytes(descs, batch):
    """qhea_model_qubit_sweep_workspace_bytes for the members' descriptors; 0 if they cannot train as one qubit sweep."""
    arr, R = _desc_array(descs)
    return int(load().qhea_model_qubit_sweep_workspace_bytes(arr, R, int(batch)))


def model_qubit_sweep_train_steps(descs, members, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq,
                                  first_step, beta1, beta2, eps, weight_decay, ham_diag=None):
    """
    model_depth_sweep_train_steps for members whose circuits also differ in qubit count (qhea_model_qubit_sweep_train_steps):
    descs is the list of R member descriptors (equal but for n_qubits and the depth entries of net).  params / exp_avg /
    exp_avg_sq: [R, Pmax]; rows: [R, n_steps, >= Pmax + 2]; ham_diag: [R, 2^nmax], member m's spectrum in the first 2^n_m entries
    of its row.  Member m gets bitwise what model_train_steps gives for it alone under the packed backward variant.
    """
    return _member_train_steps('model_qubit_sweep_train_steps', descs, members, None,
                               lambda R, b: model_qubit_sweep_workspace_bytes(descs, b),
                               "the descriptors differ in more than their qubit counts and depths",
                               lambda ds: max(d.n_qubits for d in ds),
                               bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq, first_step,
                               beta1, beta2, eps, weight_decay, ham_diag)


class Unsupported(QheaError):
    """QHEA_EUNSUPPORTED from a call that checks before it launches: the caller takes its other path."""


def model_dp_train_steps(desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq, first_step, lr,
                         beta1, beta2, eps, weight_decay, rank, world, buffers, dp_values, first_seq, timeout_ms=5000.0,
                         ham_diag=None):
    """
    model_train_steps for `world` ranks with the sum over the ranks inside each step's reduce kernel
    (qhea_model_dp_train_steps): this rank's shard rows bounds[i]:bounds[i+1] per step, exchange numbers first_seq + i on the
    peer-mapped `buffers`; rows[i] receives the GLOBAL [grads | sse | sum y^2].  Raises Unsupported -- nothing launched --
    for an empty shard or a reduce grid that would not be resident at once.
    """
    lib = load()
    if len(bounds) - 1 <= 0:
        return rows
    n_steps, rb, ib, biggest = _flat_train_schedule('model_dp_train_steps', desc, bounds, global_batches, branch, trunk, y, params,
                                                    rows, exp_avg, exp_avg_sq, ham_diag)
    ws = _model_ws(desc, biggest, branch.device)
    arr = (ctypes.c_void_p * world)(*buffers)
    with torch.cuda.device(branch.device):
        rc = lib.qhea_model_dp_train_steps(ctypes.byref(desc), n_steps, rb, _ptr(branch), _ptr(trunk), _ptr(y), _ptr(params),
                                           _ptr(ham_diag), ib, _ptr(rows), int(rows.stride(0)), _ptr(exp_avg),
                                           _ptr(exp_avg_sq), int(first_step), float(lr), float(beta1), float(beta2),
                                           float(eps), float(weight_decay), int(rank), int(world), arr, int(dp_values),
                                           int(first_seq), float(timeout_ms), _ptr(ws), ws.numel(), _stream(branch.device))
    if rc == -2:
        raise Unsupported("qhea_model_dp_train_steps: empty shard or reduce grid not resident at once")
    _check(rc, 'qhea_model_dp_train_steps')
    return rows


def _forward_noisy(wide, desc, branch, trunk, params, noise, row0, ham_diag, out, stderr):
    """The two trajectory entry points share one argument list: qhea_model_forward_noisy (n <= 6) and ..._noisy_wide (n >= 7)."""
    lib = load()
    tag, refused = ('noisy_wide', 'n <= 6') if wide else ('noisy', 'n >= 7')
    entry = f'qhea_model_forward_{tag}'
    B = _model_inputs(desc, branch, trunk, params, ham_diag)
    pred = out if out is not None else torch.empty(B, dtype=torch.float64, device=branch.device)
    ws = _sized_ws(branch.device, getattr(lib, f'qhea_model_{tag}_workspace_bytes'), ctypes.byref(desc), int(B),
                   ctypes.byref(noise))
    with torch.cuda.device(branch.device):
        rc = getattr(lib, entry)(ctypes.byref(desc), int(row0), int(B), _ptr(branch), _ptr(trunk), _ptr(params),
                                 _ptr(ham_diag), ctypes.byref(noise), _ptr(pred), _ptr(stderr), _ptr(ws),
                                 0 if ws is None else ws.numel(), _stream(branch.device))
    if rc == -2:
        raise Unsupported(f"{entry}: unsupported circuit ({refused})")
    _check(rc, entry)
    return pred, stderr


def model_forward_noisy(desc, branch, trunk, params, noise, row0=0, ham_diag=None, out=None, stderr=None):
    """
    qhea_model_forward_noisy on all rows of branch / trunk in ONE call: (pred[B], stderr[B] or None).  `noise` is a NoiseParams;
    row0 is the global index of the first row (the random streams are keyed by it).  Raises Unsupported for n >= 7 and
    QheaError for a bad noise setting -- in both cases before anything is launched.
    """
    return _forward_noisy(False, desc, branch, trunk, params, noise, row0, ham_diag, out, stderr)


def model_forward_noisy_wide(desc, branch, trunk, params, noise, row0=0, ham_diag=None, out=None, stderr=None):
    """
    qhea_model_forward_noisy_wide: model_forward_noisy for n = 7..12 -- the same arguments, quantity and random streams.  Raises
    Unsupported for n <= 6 (model_forward_noisy is the path for those) and QheaError for a bad noise setting, both before
    anything is launched.
    """
    return _forward_noisy(True, desc, branch, trunk, params, noise, row0, ham_diag, out, stderr)


def _forward_noisy_exact(device_model, desc, branch, trunk, params, noise, ham_diag, out, shot_std, wide=False):
    """The exact entry points share one argument list: qhea_model_forward_noisy_exact (`noise` a NoiseParams),
    ..._noisy_device_exact (a DeviceNoiseParams) and, with their own workspace, ..._noisy_exact_wide (a NoiseParams, n = 7..9) and
    ..._noisy_device_exact_wide (a DeviceNoiseParams, n = 7..9)."""
    lib = load()
    entry = 'qhea_model_forward_noisy' + ('_device_exact' if device_model else '_exact') + ('_wide' if wide else '')
    sizer = lib.qhea_model_device_exact_noisy_wide_workspace_bytes if wide and device_model else \
        lib.qhea_model_exact_noisy_wide_workspace_bytes if wide else lib.qhea_model_exact_noisy_workspace_bytes
    B = _model_inputs(desc, branch, trunk, params, ham_diag)
    _dev_f64(shot_std, 'shot_std', (B,))
    pred = out if out is not None else torch.empty(B, dtype=torch.float64, device=branch.device)
    ws = _sized_ws(branch.device, sizer, ctypes.byref(desc), int(B))
    with torch.cuda.device(branch.device):
        rc = getattr(lib, entry)(ctypes.byref(desc), int(B), _ptr(branch), _ptr(trunk), _ptr(params), _ptr(ham_diag),
                                 ctypes.byref(noise), _ptr(pred), _ptr(shot_std), _ptr(ws), 0 if ws is None else ws.numel(),
                                 _stream(branch.device))
    if rc == -2:
        raise Unsupported(f"{entry}: unsupported circuit ({'n <= 6 or n >= 10' if wide else 'n >= 7'})")
    _check(rc, entry)
    return pred, shot_std


def model_forward_noisy_exact(desc, branch, trunk, params, noise, ham_diag=None, out=None, shot_std=None):
    """
    qhea_model_forward_noisy_exact on all rows of branch / trunk in ONE call: (pred[B], shot_std[B] or None) -- the exact
    expectation under `noise` (a NoiseParams; p1, p2, readout are used) and, where a shot_std tensor is given, the exact
    standard deviation of one shot.  Raises Unsupported for n >= 7 and QheaError for a bad noise setting -- in both cases before
    anything is launched.
    """
    return _forward_noisy_exact(False, desc, branch, trunk, params, noise, ham_diag, out, shot_std)


def model_forward_noisy_exact_wide(desc, branch, trunk, params, noise, ham_diag=None, out=None, shot_std=None):
    """
    qhea_model_forward_noisy_exact_wide: model_forward_noisy_exact for n = 7..9 -- the same arguments and quantities, the density
    matrix of all rows in the workspace (4^n x 16 bytes per row).  Raises Unsupported for n <= 6 (model_forward_noisy_exact is
    the call for those) and n >= 10, and QheaError for a bad noise setting -- in both cases before anything is launched.
    """
    return _forward_noisy_exact(False, desc, branch, trunk, params, noise, ham_diag, out, shot_std, wide=True)


def device_noise_tables(n, noise):
    """
    qhea_device_noise_tables (host only, no device needed): (chan [4, n, 3], lam2 [n]) as numpy arrays -- the (off, a, b)
    triples of the four channel sites per wire (ENC, ROT, CTL, TGT) and 16 p2[j] / 15 per CNOT slot for `noise`, a
    DeviceNoiseParams.  Raises QheaError for a setting the library refuses.
    """
    import numpy as np
    n = int(n)
    chan = np.zeros((4, max(n, 0), 3), dtype=np.float64)
    lam2 = np.zeros(max(n, 0), dtype=np.float64)
    f64p = ctypes.POINTER(ctypes.c_double)
    _check(load().qhea_device_noise_tables(n, ctypes.byref(noise), chan.ctypes.data_as(f64p), lam2.ctypes.data_as(f64p)),
           'qhea_device_noise_tables')
    return chan, lam2


def model_forward_noisy_device_exact(desc, branch, trunk, params, noise, ham_diag=None, out=None, shot_std=None):
    """
    qhea_model_forward_noisy_device_exact on all rows of branch / trunk in ONE call: model_forward_noisy_exact with `noise` a
    DeviceNoiseParams (per-wire rates, T1 / T2, layer durations).  Raises Unsupported for n >= 7 and QheaError for a bad noise
    setting -- in both cases before anything is launched.
    """
    return _forward_noisy_exact(True, desc, branch, trunk, params, noise, ham_diag, out, shot_std)


def model_forward_noisy_device_exact_wide(desc, branch, trunk, params, noise, ham_diag=None, out=None, shot_std=None):
    """
    qhea_model_forward_noisy_device_exact_wide: model_forward_noisy_device_exact for n = 7..9 -- the same arguments (`noise` a
    DeviceNoiseParams) and quantities, the density matrix of all rows in the workspace (4^n x 16 bytes per row).  Raises
    Unsupported for n <= 6 (model_forward_noisy_device_exact is the call for those) and n >= 10, and QheaError for a bad noise
    setting -- in both cases before anything is launched.
    """
    return _forward_noisy_exact(True, desc, branch, trunk, params, noise, ham_diag, out, shot_std, wide=True)


def device_noise_jump_tables(n, noise):
    """
    qhea_device_noise_jump_tables (host only, no device needed): jump [4, n, 2] as a numpy array -- (gamma, pz) of the relaxation
    of every channel site (ENC, ROT, CTL, TGT) and wire at its folded duration, as the trajectory call unravels it, for `noise`,
    a DeviceNoiseParams.  Raises QheaError for a setting the library refuses.
    """
    import numpy as np
    n = int(n)
    jump = np.zeros((4, max(n, 0), 2), dtype=np.float64)
    _check(load().qhea_device_noise_jump_tables(n, ctypes.byref(noise), jump.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
           'qhea_device_noise_jump_tables')
    return jump


def model_noisy_device_workspace_bytes(desc, batch, sampling):
    """qhea_model_noisy_device_workspace_bytes: 0 for a bad descriptor or sampling record (a SamplingParams), or n >= 10."""
    return int(load().qhea_model_noisy_device_workspace_bytes(ctypes.byref(desc), int(batch), ctypes.byref(sampling)))


def _forward_noisy_device(entry, sizer, why, desc, branch, trunk, params, noise, sampling, row0, ham_diag, out, stderr):
    lib = load()
    B = _model_inputs(desc, branch, trunk, params, ham_diag)
    _dev_f64(stderr, 'stderr', (B,))
    pred = out if out is not None else torch.empty(B, dtype=torch.float64, device=branch.device)
    ws = _sized_ws(branch.device, getattr(lib, sizer), ctypes.byref(desc), int(B), ctypes.byref(sampling))
    with torch.cuda.device(branch.device):
        rc = getattr(lib, entry)(ctypes.byref(desc), int(row0), int(B), _ptr(branch), _ptr(trunk), _ptr(params), _ptr(ham_diag),
                                 ctypes.byref(noise), ctypes.byref(sampling), _ptr(pred), _ptr(stderr), _ptr(ws),
                                 0 if ws is None else ws.numel(), _stream(branch.device))
    if rc == -2:
        raise Unsupported(f"{entry}: unsupported circuit ({why})")
    _check(rc, entry)
    return pred, stderr


def model_forward_noisy_device(desc, branch, trunk, params, noise, sampling, row0=0, ham_diag=None, out=None, stderr=None):
    """
    qhea_model_forward_noisy_device on all rows of branch / trunk in ONE call: (pred[B], stderr[B] or None) from quantum-jump
    trajectories under `noise` (a DeviceNoiseParams) with the estimator `sampling` (a SamplingParams); row0 is the global index
    of the first row (the random streams are keyed by it).  n = 2..9: raises Unsupported for n >= 10 (that range is
    model_forward_noisy_device_wide's) and QheaError for a bad noise setting or sampling record -- in both cases before anything
    is launched.
    """
    return _forward_noisy_device('qhea_model_forward_noisy_device', 'qhea_model_noisy_device_workspace_bytes', 'n >= 10', desc,
                                 branch, trunk, params, noise, sampling, row0, ham_diag, out, stderr)


def model_noisy_device_wide_workspace_bytes(desc, batch, sampling):
    """qhea_model_noisy_device_wide_workspace_bytes: 0 for a bad descriptor or sampling record (a SamplingParams), or n <= 9."""
    return int(load().qhea_model_noisy_device_wide_workspace_bytes(ctypes.byref(desc), int(batch), ctypes.byref(sampling)))


def model_forward_noisy_device_wide(desc, branch, trunk, params, noise, sampling, row0=0, ham_diag=None, out=None, stderr=None):
    """
    model_forward_noisy_device for n = 10..12 (qhea_model_forward_noisy_device_wide: the same model, unravelling and random
    stream, the state in LDS).  Raises Unsupported for n <= 9 and QheaError for a bad noise setting or sampling record -- in both
    cases before anything is launched.
    """
    return _forward_noisy_device('qhea_model_forward_noisy_device_wide', 'qhea_model_noisy_device_wide_workspace_bytes', 'n <= 9',
                                 desc, branch, trunk, params, noise, sampling, row0, ham_diag, out, stderr)


def model_exact_noisy_log10_amplification(desc, noise):
    """
    qhea_model_exact_noisy_log10_amplification (host only): log10 of the factor by which the gradient's inverse walk amplifies
    the traceless part of rho for this shape and these rates; inf for a singular channel (p1 >= 3/4 or p2 >= 15/16), NaN for a
    bad descriptor or rates.  The gradient calls refuse values above 12.
    """
    return float(load().qhea_model_exact_noisy_log10_amplification(ctypes.byref(desc), ctypes.byref(noise)))


def _check_noisy_grad(rc, who):
    if rc == -2:
        raise Unsupported(f"{who}: n >= 7, or rates and depth whose inverse walk is ill-conditioned (log10 amplification > 12, "
                          "a lower bound under a DeviceNoise -- include/quanonet_hea.h --, or a singular channel)")
    _check(rc, who)


# The noisy gradient units by the name in their entry points (qhea_model_loss_grad_<name>, qhea_model_train_steps_<name>):
#   size, size_rec   the workspace query: called with (desc, batch) and then the record `size_rec` by reference (None: no record)
#   row0             whether loss_grad takes row0 in front of the batch
#   records          the records that go in by reference behind ham_diag, in their order
#   check            how a non-zero return code is reported: check(rc, entry, desc, records)
_GradUnit = collections.namedtuple('_GradUnit', 'size size_rec row0 records check')


def _exact_unit(size):
    return _GradUnit(size, None, False, ('noise',), lambda rc, who, desc, records: _check_noisy_grad(rc, who))


def _check_exact_wide_grad(rc, who):
    if rc == -2:
        raise Unsupported(f"{who}: the tiled density-matrix gradient is built for n = 7..9 (n <= 6: the noisy_exact calls; "
                          "n >= 10: the sampled noisy_lds calls), or rates and depth whose inverse walk is ill-conditioned "
                          "(log10 amplification > 12, or a singular channel)")
    _check(rc, who)


def _check_device_exact_wide_grad(rc, who):
    if rc == -2:
        raise Unsupported(f"{who}: the tiled device-noise gradient is built for n = 7..9 (n <= 6: the noisy_device_exact calls; "
                          "n >= 10: the sampled noisy_device_lds calls), or a setting and depth whose inverse walk is "
                          "ill-conditioned (log10 A_dev > 7, or a singular channel)")
    _check(rc, who)


def _check_device_exact_wide_stored_grad(rc, who):
    if rc == -2:
        raise Unsupported(f"{who}: the tiled stored-state device-noise gradient is built for n = 7..9 (n <= 6: the "
                          "noisy_device_exact_stored calls; n >= 10: the sampled noisy_device_lds calls), or a setting whose "
                          "largest single unit is ill-conditioned (layer log10 A_dev > 7, or a singular channel)")
    _check(rc, who)


def _sampled_unit(kind):
    return _GradUnit(f'qhea_model_noisy_{kind}_grad_workspace_bytes', 'noise', True, ('noise',),
                     lambda rc, who, desc, records: _check_noisy_wide_grad(rc, who, kind))


def _jump_unit(size):
    return _GradUnit(size, 'sampling', True, ('noise', 'sampling'),
                     lambda rc, who, desc, records: _check_device_sampled(rc, who, desc, records['noise']))


_GRAD_UNITS = {'noisy_exact': _exact_unit('qhea_model_exact_noisy_grad_workspace_bytes'),
               'noisy_exact_wide': _GradUnit('qhea_model_exact_noisy_wide_grad_workspace_bytes', None, False, ('noise',),
                                             lambda rc, who, desc, records: _check_exact_wide_grad(rc, who)),
               'noisy_device_exact': _exact_unit('qhea_model_device_noisy_grad_workspace_bytes'),
               'noisy_device_exact_stored': _exact_unit('qhea_model_device_noisy_stored_grad_workspace_bytes'),
               'noisy_device_exact_wide': _GradUnit('qhea_model_device_noisy_wide_grad_workspace_bytes', None, False, ('noise',),
                                                    lambda rc, who, desc, records: _check_device_exact_wide_grad(rc, who)),
               'noisy_device_exact_wide_stored': _GradUnit('qhea_model_device_noisy_wide_stored_grad_workspace_bytes', None, False,
                                                           ('noise',), lambda rc, who, desc, records:
                                                           _check_device_exact_wide_stored_grad(rc, who)),
               'noisy_wide': _sampled_unit('wide'),
               'noisy_lds': _sampled_unit('lds'),
               'noisy_device': _jump_unit('qhea_model_noisy_device_grad_workspace_bytes'),
               'noisy_device_lds': _jump_unit('qhea_model_noisy_device_lds_grad_workspace_bytes')}


def _grad_unit_ws(lib, unit, desc, B, records, device):
    rec = () if unit.size_rec is None else (ctypes.byref(records[unit.size_rec]),)
    return _sized_ws(device, getattr(lib, unit.size), ctypes.byref(desc), int(B), *rec)


def _loss_grad_call(name, desc, branch, trunk, y, params, records, inv_batch_total, grad, row0, ham_diag, pred):
    """qhea_model_loss_grad_<name> of a unit of _GRAD_UNITS; `records`: its records by name"""
    lib = load()
    unit, entry = _GRAD_UNITS[name], 'qhea_model_loss_grad_' + name
    B = _model_inputs(desc, branch, trunk, params, ham_diag)
    _dev_f64(y, 'y')
    if y.numel() != B:
        raise QheaError(f"y has {y.numel()} elements, expected {B}")
    _dev_f64(grad, 'grad')
    if grad.numel() < params.numel() + 2:
        raise QheaError(f"{entry[5:]}: grad needs P + 2 entries")
    _dev_f64(pred, 'pred', (B,))
    ws = _grad_unit_ws(lib, unit, desc, B, records, branch.device)
    rows = (int(row0), B) if unit.row0 else (B,)
    with torch.cuda.device(branch.device):
        rc = getattr(lib, entry)(ctypes.byref(desc), *rows, _ptr(branch), _ptr(trunk), _ptr(y), _ptr(params), _ptr(ham_diag),
                                 *(ctypes.byref(records[k]) for k in unit.records), float(inv_batch_total), _ptr(grad),
                                 _ptr(pred), _ptr(ws), 0 if ws is None else ws.numel(), _stream(branch.device))
    unit.check(rc, entry, desc, records)
    return grad


def _train_steps_call(name, desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq, first_step, lr,
                      beta1, beta2, eps, weight_decay, records, ham_diag):
    """qhea_model_train_steps_<name> of a unit of _GRAD_UNITS; `records`: its records by name"""
    lib = load()
    unit, entry = _GRAD_UNITS[name], 'qhea_model_train_steps_' + name
    if len(bounds) - 1 <= 0:
        return rows
    n_steps, rb, ib, biggest = _flat_train_schedule(entry[5:], desc, bounds, global_batches, branch, trunk, y, params, rows,
                                                    exp_avg, exp_avg_sq, ham_diag)
    ws = _grad_unit_ws(lib, unit, desc, biggest, records, branch.device)
    with torch.cuda.device(branch.device):
        rc = getattr(lib, entry)(ctypes.byref(desc), n_steps, rb, _ptr(branch), _ptr(trunk), _ptr(y), _ptr(params),
                                 _ptr(ham_diag), *(ctypes.byref(records[k]) for k in unit.records), ib, _ptr(rows),
                                 int(rows.stride(0)), _ptr(exp_avg), _ptr(exp_avg_sq), int(first_step), float(lr), float(beta1),
                                 float(beta2), float(eps), float(weight_decay), _ptr(ws), 0 if ws is None else ws.numel(),
                                 _stream(branch.device))
    unit.check(rc, entry, desc, records)
    return rows


def model_loss_grad_noisy_exact(desc, branch, trunk, y, params, noise, inv_batch_total, grad, ham_diag=None, pred=None):
    """
    model_loss_grad under `noise` (a NoiseParams; p1, p2, readout are used): fills grad[P+2] = [d loss/d params | sse | sum y^2]
    of the exact noisy prediction for this shard (qhea_model_loss_grad_noisy_exact); returns grad.  Raises Unsupported for
    n >= 7 or a refused conditioning and QheaError for a bad noise setting, in both cases before anything is launched.
    """
    return _loss_grad_call('noisy_exact', desc, branch, trunk, y, params, dict(noise=noise), inv_batch_total, grad, 0, ham_diag,
                           pred)


def model_train_steps_noisy_exact(desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq, first_step,
                                  lr, beta1, beta2, eps, weight_decay, noise, ham_diag=None):
    """
    model_train_steps with the noise in the loss (qhea_model_train_steps_noisy_exact): step i trains on rows
    bounds[i]:bounds[i+1] under `noise` with residual weight 1 / global_batches[i], leaves [grads | sse | sum y^2] in rows[i]
    and applies Adam update first_step + i.  Bitwise a loop of model_loss_grad_noisy_exact + adam_step.
    """
    return _train_steps_call('noisy_exact', desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq,
                             first_step, lr, beta1, beta2, eps, weight_decay, dict(noise=noise), ham_diag)


def model_exact_noisy_wide_grad_workspace_bytes(desc, batch):
    """qhea_model_exact_noisy_wide_grad_workspace_bytes: 0 for a bad descriptor or n outside 7..9."""
    return int(load().qhea_model_exact_noisy_wide_grad_workspace_bytes(ctypes.byref(desc), int(batch)))


def model_loss_grad_noisy_exact_wide(desc, branch, trunk, y, params, noise, inv_batch_total, grad, ham_diag=None, pred=None):
    """model_loss_grad_noisy_exact for n = 7..9 (qhea_model_loss_grad_noisy_exact_wide): rho and O tiled through the workspace."""
    return _loss_grad_call('noisy_exact_wide', desc, branch, trunk, y, params, dict(noise=noise), inv_batch_total, grad, 0,
                           ham_diag, pred)


def model_train_steps_noisy_exact_wide(desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq,
                                       first_step, lr, beta1, beta2, eps, weight_decay, noise, ham_diag=None):
    """model_train_steps_noisy_exact for n = 7..9 (qhea_model_train_steps_noisy_exact_wide)."""
    return _train_steps_call('noisy_exact_wide', desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg,
                             exp_avg_sq, first_step, lr, beta1, beta2, eps, weight_decay, dict(noise=noise), ham_diag)


def model_noisy_wide_grad_workspace_bytes(desc, batch, noise):
    """qhea_model_noisy_wide_grad_workspace_bytes: 0 for a bad descriptor or noise setting (shot mode included) or n outside 7..9."""
    return int(load().qhea_model_noisy_wide_grad_workspace_bytes(ctypes.byref(desc), int(batch), ctypes.byref(noise)))


# The two sampled-trajectory gradient pairs share their arguments: `kind` is 'wide' (n = 7..9) or 'lds' (n = 10..12)
_SAMPLED_RANGE = {'wide': "n outside 7..9 (n <= 6: the exact calls; n >= 10: the _lds calls)",
                  'lds': "n outside 10..12 (n = 7..9: the _wide calls; n <= 6: the exact calls)"}


def _check_noisy_wide_grad(rc, who, kind='wide'):
    if rc == -2:
        raise Unsupported(f"{who}: {_SAMPLED_RANGE[kind]}")
    _check(rc, who)


def model_loss_grad_noisy_wide(desc, branch, trunk, y, params, noise, inv_batch_total, grad, row0=0, ham_diag=None, pred=None):
    """
    model_loss_grad of the SAMPLED noisy prediction (qhea_model_loss_grad_noisy_wide, n = 7..9): fills grad[P+2] =
    [d loss/d params | sse | sum y^2] where pred is what model_forward_noisy_wide returns for the same `noise` (a NoiseParams in
    expectation mode: trajectories and seed are used) and global rows row0 + b, differentiated with the random stream held
    fixed; returns grad.  Raises Unsupported for n outside 7..9 and QheaError for a bad noise setting (shots > 0 included), in
    both cases before anything is launched.
    """
    return _loss_grad_call('noisy_wide', desc, branch, trunk, y, params, dict(noise=noise), inv_batch_total, grad, row0, ham_diag,
                           pred)


def model_train_steps_noisy_wide(desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq, first_step,
                                 lr, beta1, beta2, eps, weight_decay, noise, ham_diag=None):
    """
    model_train_steps with the sampled noisy loss (qhea_model_train_steps_noisy_wide, n = 7..9): step i trains on rows
    bounds[i]:bounds[i+1] (their global row indices key the random stream) under `noise` with the seed noise.seed +
    first_step + i, leaves [grads | sse | sum y^2] in rows[i] and applies Adam update first_step + i.  Bitwise a loop of
    model_loss_grad_noisy_wide (that seed, row0 = bounds[i]) + adam_step.
    """
    return _train_steps_call('noisy_wide', desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq,
                             first_step, lr, beta1, beta2, eps, weight_decay, dict(noise=noise), ham_diag)


def model_noisy_lds_grad_workspace_bytes(desc, batch, noise):
    """qhea_model_noisy_lds_grad_workspace_bytes: 0 for a bad descriptor or noise setting (shot mode included) or n outside 10..12."""
    return int(load().qhea_model_noisy_lds_grad_workspace_bytes(ctypes.byref(desc), int(batch), ctypes.byref(noise)))


def model_loss_grad_noisy_lds(desc, branch, trunk, y, params, noise, inv_batch_total, grad, row0=0, ham_diag=None, pred=None):
    """model_loss_grad_noisy_wide at n = 10..12 (qhea_model_loss_grad_noisy_lds): same arguments, same quantity, psi and lambda
    in LDS.  Raises Unsupported for n outside 10..12."""
    return _loss_grad_call('noisy_lds', desc, branch, trunk, y, params, dict(noise=noise), inv_batch_total, grad, row0, ham_diag,
                           pred)


def model_train_steps_noisy_lds(desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq, first_step,
                                lr, beta1, beta2, eps, weight_decay, noise, ham_diag=None):
    """model_train_steps_noisy_wide at n = 10..12 (qhea_model_train_steps_noisy_lds): bitwise a loop of
    model_loss_grad_noisy_lds (seed noise.seed + first_step + i, row0 = bounds[i]) + adam_step."""
    return _train_steps_call('noisy_lds', desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq,
                             first_step, lr, beta1, beta2, eps, weight_decay, dict(noise=noise), ham_diag)


def model_noisy_device_grad_workspace_bytes(desc, batch, sampling):
    """qhea_model_noisy_device_grad_workspace_bytes: 0 for a bad descriptor or sampling record (shot mode included) or n outside 7..9."""
    return int(load().qhea_model_noisy_device_grad_workspace_bytes(ctypes.byref(desc), int(batch), ctypes.byref(sampling)))


SITE_NAMES = ('ENC', 'ROT', 'CTL', 'TGT')


def device_noise_singular_site(n, noise):
    """qhea_device_noise_singular_site (host only): (site name, wire) of the first relaxation site of `noise` (a DeviceNoiseParams)
    with 1 - gamma == 0, which the trajectory gradient cannot walk back, or None."""
    site, wire = ctypes.c_int(0), ctypes.c_int(0)
    rc = load().qhea_device_noise_singular_site(int(n), ctypes.byref(noise), ctypes.byref(site), ctypes.byref(wire))
    if rc < 0:
        _check(rc, 'qhea_device_noise_singular_site')
    return (SITE_NAMES[site.value], wire.value) if rc == 1 else None


def model_noisy_device_lds_grad_workspace_bytes(desc, batch, sampling):
    """qhea_model_noisy_device_lds_grad_workspace_bytes: 0 for a bad descriptor or sampling record (shot mode included) or n outside
    10..12."""
    return int(load().qhea_model_noisy_device_lds_grad_workspace_bytes(ctypes.byref(desc), int(batch), ctypes.byref(sampling)))


def noisy_device_lds_grad_max_workgroups(n):
    """qhea_noisy_device_lds_grad_max_workgroups: the workgroups one launch of the n = 10..12 quantum-jump gradient kernel has at
    most (more (row, tile) items go round its grid-stride loop); 0 outside 10..12."""
    return int(load().qhea_noisy_device_lds_grad_max_workgroups(int(n)))


def _check_device_sampled(rc, who, desc, noise):
    if rc == -2:
        if who.endswith('_lds'):
            raise Unsupported(f"{who}: n outside 10..12 (n <= 6: the exact calls under a device noise model; n = 7..9: "
                              f"{who[:-4]})")
        raise Unsupported(f"{who}: n outside 7..9 (n <= 6: the exact calls under a device noise model; n >= 10: {who}_lds)")
    if rc == -1:
        hit = None
        try:
            hit = device_noise_singular_site(desc.n_qubits, noise)
        except QheaError:
            pass
        if hit:
            raise QheaError(f"{who}: relaxation site {hit[0]} on wire {hit[1]} has gamma = 1 (1 - gamma == 0 in fp64): the "
                            "trajectory gradient cannot walk it back")
    _check(rc, who)


def model_loss_grad_noisy_device(desc, branch, trunk, y, params, noise, sampling, inv_batch_total, grad, row0=0, ham_diag=None,
                                 pred=None):
    """
    model_loss_grad of the quantum-jump estimate under `noise` (a DeviceNoiseParams) with the estimator `sampling` (a
    SamplingParams in expectation mode), n = 7..9 (qhea_model_loss_grad_noisy_device): fills grad[P+2] = [d loss/d params | sse |
    sum y^2] where pred is what model_forward_noisy_device returns for the same arguments and global rows row0 + b, and
    d pred / d params is the unbiased estimate stated in include/quanonet_hea.h (the unnormalised numerator's gradient with the
    fired pattern fixed, over the final norm); returns grad.  Raises Unsupported for n outside 7..9 and QheaError for a bad
    setting (shots != 0 and a site with gamma = 1 included), in both cases before anything is launched.
    """
    return _loss_grad_call('noisy_device', desc, branch, trunk, y, params, dict(noise=noise, sampling=sampling), inv_batch_total,
                           grad, row0, ham_diag, pred)


def model_loss_grad_noisy_device_lds(desc, branch, trunk, y, params, noise, sampling, inv_batch_total, grad, row0=0, ham_diag=None,
                                     pred=None):
    """model_loss_grad_noisy_device for n = 10..12 (qhea_model_loss_grad_noisy_device_lds: the same quantity, estimator and
    random stream with psi and lambda in LDS; pred is what model_forward_noisy_device_wide returns).  Same errors, with the
    qubit range 10..12."""
    return _loss_grad_call('noisy_device_lds', desc, branch, trunk, y, params, dict(noise=noise, sampling=sampling),
                           inv_batch_total, grad, row0, ham_diag, pred)


def model_train_steps_noisy_device(desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq, first_step,
                                   lr, beta1, beta2, eps, weight_decay, noise, sampling, ham_diag=None):
    """
    model_train_steps with the quantum-jump loss under a device noise model (qhea_model_train_steps_noisy_device, n = 7..9): step
    i trains on rows bounds[i]:bounds[i+1] (their global row indices key the random stream) with the stream key sampling.seed +
    first_step + i, leaves [grads | sse | sum y^2] in rows[i] and applies Adam update first_step + i.  Bitwise a loop of
    model_loss_grad_noisy_device (that seed, row0 = bounds[i]) + adam_step.
    """
    return _train_steps_call('noisy_device', desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq,
                             first_step, lr, beta1, beta2, eps, weight_decay, dict(noise=noise, sampling=sampling), ham_diag)


def model_train_steps_noisy_device_lds(desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq,
                                       first_step, lr, beta1, beta2, eps, weight_decay, noise, sampling, ham_diag=None):
    """model_train_steps_noisy_device for n = 10..12 (qhea_model_train_steps_noisy_device_lds).  Bitwise a loop of
    model_loss_grad_noisy_device_lds (seed sampling.seed + first_step + i, row0 = bounds[i]) + adam_step."""
    return _train_steps_call('noisy_device_lds', desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq,
                             first_step, lr, beta1, beta2, eps, weight_decay, dict(noise=noise, sampling=sampling), ham_diag)


def sampled_grad_calls(n):
    """(loss_grad, train_steps) of the sampled-trajectory gradient for n qubits: the wave-resident unit (model_*_noisy_wide,
    n = 7..9) or the LDS-resident one (model_*_noisy_lds, n = 10..12); the calls themselves refuse an n outside their range"""
    return ((model_loss_grad_noisy_wide, model_train_steps_noisy_wide) if n <= 9 else
            (model_loss_grad_noisy_lds, model_train_steps_noisy_lds))


def device_sampled_grad_calls(n):
    """sampled_grad_calls for the quantum-jump gradient under a device noise model: model_*_noisy_device (n = 7..9) or
    model_*_noisy_device_lds (n = 10..12)"""
    return ((model_loss_grad_noisy_device, model_train_steps_noisy_device) if n <= 9 else
            (model_loss_grad_noisy_device_lds, model_train_steps_noisy_device_lds))


def model_device_noisy_log10_amplification(desc, noise):
    """
    qhea_model_device_noisy_log10_amplification (host only): log10 A_dev of this shape under `noise` (a DeviceNoiseParams) --
    what the inverse walk of the device-noise gradient amplifies the traceless part of rho by; inf for a singular channel,
    NaN for a bad descriptor or a setting the library refuses.  The gradient calls refuse values above their bound
    (model_device_noisy_refused answers for a model and a setting).
    """
    return float(load().qhea_model_device_noisy_log10_amplification(ctypes.byref(desc), ctypes.byref(noise)))


def model_device_noisy_log10_layer_amplification(desc, noise):
    """
    qhea_model_device_noisy_log10_layer_amplification (host only): log10 A_dev of the largest single unit of this shape under
    `noise` (a DeviceNoiseParams) -- one sub-layer's sites and slots with the encoding sites -- which is what the stored-state
    gradient calls are bounded by; inf and NaN where model_device_noisy_log10_amplification returns them.
    """
    return float(load().qhea_model_device_noisy_log10_layer_amplification(ctypes.byref(desc), ctypes.byref(noise)))


def model_device_noisy_stored_grad_workspace_bytes(desc, batch, snapshots_only=False):
    """qhea_model_device_noisy_stored_grad_workspace_bytes (host only): the inverse walk's workspace plus the snapshot region
    (units x batch x 16 x 4^n bytes, rounded up to 256); snapshots_only: the region alone."""
    lib = load()
    total = int(lib.qhea_model_device_noisy_stored_grad_workspace_bytes(ctypes.byref(desc), int(batch)))
    return total - int(lib.qhea_model_device_noisy_grad_workspace_bytes(ctypes.byref(desc), int(batch))) if snapshots_only else total


def _device_noisy_refused(entry, desc, noise):
    rc = getattr(load(), entry)(ctypes.byref(desc), 0, None, None, None, None, None, ctypes.byref(noise), 1.0, None, None, None, 0,
                                None)
    if rc == -2:
        return True
    _check(rc, entry)
    return False


def model_device_noisy_stored_refused(desc, noise):
    """
    model_device_noisy_refused for the stored-state calls (qhea_model_loss_grad_noisy_device_exact_stored): n >= 7, a singular
    channel, or a layer amplification above the library's bound -- the total amplification is no reason.  Host only.
    """
    return _device_noisy_refused('qhea_model_loss_grad_noisy_device_exact_stored', desc, noise)


def model_device_noisy_refused(desc, noise):
    """
    Whether the device-noise gradient calls refuse this model under `noise` (a DeviceNoiseParams) with QHEA_EUNSUPPORTED --
    n >= 7, a singular channel, or log10 A_dev above the library's bound.  Asked of the library itself: the call on an empty
    batch runs every check in front of the batch and launches nothing (host only, no device needed).  Raises QheaError for a
    setting the library refuses as invalid.
    """
    return _device_noisy_refused('qhea_model_loss_grad_noisy_device_exact', desc, noise)


def model_loss_grad_noisy_device_exact(desc, branch, trunk, y, params, noise, inv_batch_total, grad, ham_diag=None, pred=None):
    """
    model_loss_grad_noisy_exact with `noise` a DeviceNoiseParams (qhea_model_loss_grad_noisy_device_exact): loss and exact
    gradient of the prediction of model_forward_noisy_device_exact.  Same errors.
    """
    return _loss_grad_call('noisy_device_exact', desc, branch, trunk, y, params, dict(noise=noise), inv_batch_total, grad, 0,
                           ham_diag, pred)


def model_train_steps_noisy_device_exact(desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq,
                                         first_step, lr, beta1, beta2, eps, weight_decay, noise, ham_diag=None):
    """
    model_train_steps_noisy_exact with `noise` a DeviceNoiseParams (qhea_model_train_steps_noisy_device_exact).  Bitwise a loop
    of model_loss_grad_noisy_device_exact + adam_step.
    """
    return _train_steps_call('noisy_device_exact', desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg,
                             exp_avg_sq, first_step, lr, beta1, beta2, eps, weight_decay, dict(noise=noise), ham_diag)


def model_loss_grad_noisy_device_exact_stored(desc, branch, trunk, y, params, noise, inv_batch_total, grad, ham_diag=None,
                                              pred=None):
    """
    model_loss_grad_noisy_device_exact with rho replayed from stored states (qhea_model_loss_grad_noisy_device_exact_stored):
    the same quantity for settings past that call's guard; Unsupported for n >= 7, a singular channel or a single unit whose
    log10 A_dev is above the bound.  The workspace grows by units x rows x 16 x 4^n bytes.
    """
    return _loss_grad_call('noisy_device_exact_stored', desc, branch, trunk, y, params, dict(noise=noise), inv_batch_total, grad, 0,
                           ham_diag, pred)


def model_train_steps_noisy_device_exact_stored(desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq,
                                                first_step, lr, beta1, beta2, eps, weight_decay, noise, ham_diag=None):
    """
    model_train_steps_noisy_device_exact with rho replayed from stored states
    (qhea_model_train_steps_noisy_device_exact_stored).  Bitwise a loop of model_loss_grad_noisy_device_exact_stored + adam_step.
    """
    return _train_steps_call('noisy_device_exact_stored', desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg,
                             exp_avg_sq, first_step, lr, beta1, beta2, eps, weight_decay, dict(noise=noise), ham_diag)


def model_device_noisy_wide_grad_workspace_bytes(desc, batch):
    """qhea_model_device_noisy_wide_grad_workspace_bytes: 0 for a bad descriptor, a negative batch or n outside 7..9."""
    return int(load().qhea_model_device_noisy_wide_grad_workspace_bytes(ctypes.byref(desc), int(batch)))


def model_device_noisy_wide_refused(desc, noise):
    """
    model_device_noisy_refused for the tiled calls (qhea_model_loss_grad_noisy_device_exact_wide): n outside 7..9, a singular
    channel, or log10 A_dev above the library's bound.  Host only.
    """
    return _device_noisy_refused('qhea_model_loss_grad_noisy_device_exact_wide', desc, noise)


def model_loss_grad_noisy_device_exact_wide(desc, branch, trunk, y, params, noise, inv_batch_total, grad, ham_diag=None,
                                            pred=None):
    """
    model_loss_grad_noisy_device_exact for n = 7..9 (qhea_model_loss_grad_noisy_device_exact_wide): rho and O tiled through the
    workspace; pred is bitwise what model_forward_noisy_device_exact_wide returns.
    """
    return _loss_grad_call('noisy_device_exact_wide', desc, branch, trunk, y, params, dict(noise=noise), inv_batch_total, grad, 0,
                           ham_diag, pred)


def model_train_steps_noisy_device_exact_wide(desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg, exp_avg_sq,
                                              first_step, lr, beta1, beta2, eps, weight_decay, noise, ham_diag=None):
    """
    model_train_steps_noisy_device_exact for n = 7..9 (qhea_model_train_steps_noisy_device_exact_wide).  Bitwise a loop of
    model_loss_grad_noisy_device_exact_wide + adam_step.
    """
    return _train_steps_call('noisy_device_exact_wide', desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg,
                             exp_avg_sq, first_step, lr, beta1, beta2, eps, weight_decay, dict(noise=noise), ham_diag)


def model_device_noisy_wide_stored_grad_workspace_bytes(desc, batch, snapshots_only=False):
    """qhea_model_device_noisy_wide_stored_grad_workspace_bytes (host only): the tiled inverse walk's workspace plus the snapshot
    region (units x batch x 16 x 4^n bytes, rounded up to 256); snapshots_only: the region alone.  0 for a bad descriptor, a
    negative batch or n outside 7..9."""
    lib = load()
    total = int(lib.qhea_model_device_noisy_wide_stored_grad_workspace_bytes(ctypes.byref(desc), int(batch)))
    return total - int(lib.qhea_model_device_noisy_wide_grad_workspace_bytes(ctypes.byref(desc), int(batch))) if snapshots_only else total


def model_device_noisy_wide_stored_refused(desc, noise):
    """
    model_device_noisy_refused for the tiled stored-state calls (qhea_model_loss_grad_noisy_device_exact_wide_stored): n outside
    7..9, a singular channel, or a layer amplification above the library's bound -- the total amplification is no reason.
    Host only.
    """
    return _device_noisy_refused('qhea_model_loss_grad_noisy_device_exact_wide_stored', desc, noise)


def model_loss_grad_noisy_device_exact_wide_stored(desc, branch, trunk, y, params, noise, inv_batch_total, grad, ham_diag=None,
                                                   pred=None):
    """
    model_loss_grad_noisy_device_exact_wide with rho replayed from stored states
    (qhea_model_loss_grad_noisy_device_exact_wide_stored): the same quantity for settings past that call's guard; pred is bitwise
    that call's.  The workspace grows by units x rows x 16 x 4^n bytes.
    """
    return _loss_grad_call('noisy_device_exact_wide_stored', desc, branch, trunk, y, params, dict(noise=noise), inv_batch_total,
                           grad, 0, ham_diag, pred)


def model_train_steps_noisy_device_exact_wide_stored(desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg,
                                                     exp_avg_sq, first_step, lr, beta1, beta2, eps, weight_decay, noise,
                                                     ham_diag=None):
    """
    model_train_steps_noisy_device_exact_wide with rho replayed from stored states
    (qhea_model_train_steps_noisy_device_exact_wide_stored).  Bitwise a loop of model_loss_grad_noisy_device_exact_wide_stored +
    adam_step.
    """
    return _train_steps_call('noisy_device_exact_wide_stored', desc, bounds, global_batches, branch, trunk, y, params, rows, exp_avg,
                             exp_avg_sq, first_step, lr, beta1, beta2, eps, weight_decay, dict(noise=noise), ham_diag)


def clock_probe(device, n_workgroups=1024, iters=200000):
    """In-kernel shader clock in MHz (median over `n_workgroups` one-wave workgroups timing a dependent fp64 FMA chain against
    the constant 100 MHz counter; qhea_clock_probe).  A diagnostic: the latency-bound kernels scale with it."""
    buf = torch.zeros(2 * n_workgroups, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _check(load().qhea_clock_probe(int(n_workgroups), int(iters), ctypes.c_void_p(buf.data_ptr()), _stream(device)),
               'qhea_clock_probe')
    t = buf.cpu().numpy().reshape(-1, 2).astype('float64')
    mhz = 100.0 * t[:, 0] / t[:, 1]
    import numpy as _np
    return float(_np.median(mhz)), float(mhz.min()), float(mhz.max())


def profile_next_circuit_kernel(start_event, stop_event):
    """Arm the measurement hook with two torch.cuda.Event(enable_timing=True) (already recorded once)."""
    rc = load().qhea_profile_next_circuit_kernel(ctypes.c_void_p(start_event.cuda_event),
                                                 ctypes.c_void_p(stop_event.cuda_event))
    _check(rc, 'qhea_profile_next_circuit_kernel')


def adam_step(params, grads, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """In-place Adam update of the flat fp64 parameter vector (one launch); grads may be a longer buffer."""
    n = params.numel()
    for t, nm in ((params, 'params'), (grads, 'grads'), (exp_avg, 'exp_avg'), (exp_avg_sq, 'exp_avg_sq')):
        _dev_f64(t, nm)
    if grads.numel() < n or exp_avg.numel() != n or exp_avg_sq.numel() != n:
        raise QheaError("adam_step: buffer sizes do not match the parameter vector")
    with torch.cuda.device(params.device):
        rc = load().qhea_adam_step(n, _ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), int(step),
                                   float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                   _stream(params.device))
    _check(rc, 'qhea_adam_step')


# ---- data-parallel exchange (include/quanonet_hea.h: qhea_dp_*) -------------------------------------------------
DP_MAX_RANKS, DP_HANDLE_BYTES = 16, 64


def dp_alloc(n_values, world, device):
    """This rank's exchange buffer (fine-grained device memory owned by the caller): its device address."""
    p = ctypes.c_void_p()
    with torch.cuda.device(device):
        _check(load().qhea_dp_alloc(int(n_values), int(world), ctypes.byref(p)), 'qhea_dp_alloc')
    return p.value


def dp_free(buf, device):
    with torch.cuda.device(device):
        _check(load().qhea_dp_free(buf), 'qhea_dp_free')


def dp_export(buf, device):
    h = ctypes.create_string_buffer(DP_HANDLE_BYTES)
    with torch.cuda.device(device):
        _check(load().qhea_dp_export(buf, h), 'qhea_dp_export')
    return h.raw


def dp_import(handle, device):
    p = ctypes.c_void_p()
    with torch.cuda.device(device):
        _check(load().qhea_dp_import(bytes(handle), ctypes.byref(p)), 'qhea_dp_import')
    return p.value


def dp_close(peer_buf, device):
    with torch.cuda.device(device):
        _check(load().qhea_dp_close(peer_buf), 'qhea_dp_close')


def dp_allreduce_adam(rank, world, buffers, seq, local, out, params=None, exp_avg=None, exp_avg_sq=None, step=1,
                      lr=0.0, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, timeout_ms=5000.0):
    """out = sum over ranks (in rank order) of every rank's `local`; Adam on `params` with out[:params.numel()]."""
    _dev_f64(local, 'local'); _dev_f64(out, 'out')
    n = local.numel()
    if out.numel() != n:
        raise QheaError("dp_allreduce_adam: local and out differ in size")
    npar = 0
    if params is not None:
        for t, nm in ((params, 'params'), (exp_avg, 'exp_avg'), (exp_avg_sq, 'exp_avg_sq')):
            _dev_f64(t, nm)
        npar = params.numel()
        if npar > n or exp_avg.numel() != npar or exp_avg_sq.numel() != npar:
            raise QheaError("dp_allreduce_adam: buffer sizes do not match the parameter vector")
    arr = (ctypes.c_void_p * world)(*buffers)
    with torch.cuda.device(local.device):
        rc = load().qhea_dp_allreduce_adam(
            int(rank), int(world), arr, n, int(seq), _ptr(local), _ptr(out), npar,
            _ptr(params) if params is not None else None, _ptr(exp_avg) if params is not None else None,
            _ptr(exp_avg_sq) if params is not None else None, int(step), float(lr), float(beta1), float(beta2),
            float(eps), float(weight_decay), float(timeout_ms), _stream(local.device))
    _check(rc, 'qhea_dp_allreduce_adam')


def dp_status(buf, device):
    """Waits for the device's current stream; raises QheaError(QHEA_EEXCHANGE) if an exchange timed out."""
    with torch.cuda.device(device):
        _check(load().qhea_dp_status(buf, _stream(device)), 'qhea_dp_status')
