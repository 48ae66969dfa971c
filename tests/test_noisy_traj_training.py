"""
Sampled-trajectory noise-aware training through the Python layers: quanonet_amd.noise.noisy_loss_and_grad against the numpy
reference, and DataParallelTrainer / PTSolver with train_noise + train_sampling at n = 7 (qhea_model_train_steps_noisy_wide):
the run, its reproducibility, the per-step path, and every refusal.  What needs no device is not marked gpu.
"""
import numpy as np
import pytest
import torch

from tests import noisy_traj_grad_reference as TG
from tests.test_noisy_forward import _solver_data
from tests.test_noisy_traj_grad_reference import build, inputs, noise_model

gpu = pytest.mark.gpu
quiet = lambda *a, **k: None


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _cfg(tmp_path, name, **kw):
    cfg = {'model_type': 'QuanONet', 'operator': 'Toy', 'num_qubits': 7, 'net_size': [2, 1, 1, 1], 'scale_coeff': 0.5,
           'if_trainable_freq': 'true', 'learning_rate': 2e-2, 'batch_size': 100, 'num_epochs': 2, 'seed': 0,
           'prefix': str(tmp_path / name), 'run_id': 'r0', 'eval_batch_size': 64, 'trace_steps': True, 'if_save': False}
    cfg.update(kw)
    return cfg


NOISE = {'p1': 0.02, 'p2': 0.05, 'readout': 0.03}


@gpu
def test_noisy_loss_and_grad(dev):
    from quanonet_amd.noise import DeviceNoise, NoiseModel, noisy_loss_and_grad
    for kind, n, readout in (('quanonet', 7, 'X'), ('heaqnn', 8, 'diag')):
        cpu = build(kind, n, True, readout, seed=2)
        ins, y = inputs(kind, 6, seed=2), np.random.default_rng(2).normal(size=6)
        nz = noise_model((0.05, 0.1, 0.05), T=17, seed=21)
        ref, _ = TG.model_loss_grad(cpu, ins, y, 1.0 / 6, TG.TrajEngine(nz, 40))
        m = cpu.to(dev)
        dins = tuple(torch.tensor(t, device=dev) for t in ins)
        got = noisy_loss_and_grad(m, dins, torch.tensor(y, device=dev).reshape(-1, 1), nz, row0=40)
        torch.cuda.synchronize()
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=0, atol=1e-10)
        ref9, _ = TG.model_loss_grad(cpu.cpu(), ins, y, 1.0 / 9, TG.TrajEngine(nz, 0))
        got9 = noisy_loss_and_grad(cpu.to(dev), dins, torch.tensor(y, device=dev), nz, inv_batch_total=1.0 / 9)
        np.testing.assert_allclose(got9.cpu().numpy(), ref9, rtol=0, atol=1e-10)
    # refused inputs
    m = build('heaqnn', 7, True, 'Z').to(dev)
    x, y = (torch.tensor(inputs('heaqnn', 4)[0], device=dev),), torch.zeros(4, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match='shots'):
        noisy_loss_and_grad(m, x, y, NoiseModel(p1=0.01, shots=100))
    with pytest.raises(ValueError, match='DeviceNoise'):
        noisy_loss_and_grad(m, x, y, DeviceNoise(p1=0.01))
    with pytest.raises(ValueError, match='exact_noisy_loss_and_grad'):
        noisy_loss_and_grad(build('heaqnn', 6, True, 'Z').to(dev), x, y, NoiseModel(p1=0.01))
    with pytest.raises(ValueError, match='7..9'):
        noisy_loss_and_grad(build('heaqnn', 10, True, 'Z').to(dev), x, y, NoiseModel(p1=0.01))
    assert noisy_loss_and_grad(m, (x[0][:0],), y[:0], NoiseModel(p1=0.01)).abs().sum().item() == 0.0       # an empty batch


def _run(tmp_path, name, dev, seed=0, **kw):
    from quanonet_amd.solver import PTSolver, set_random_seed
    set_random_seed(seed)
    lines = []
    s = PTSolver(_cfg(tmp_path, name, **kw), _solver_data(), device=dev, log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    return s, s.train(), lines


@gpu
def test_ptsolver_train_sampling(dev, tmp_path):
    from quanonet_amd.noise import NoiseModel, Sampling
    sp = Sampling(trajectories=8, seed=11)
    s, hist, lines = _run(tmp_path, 'a', dev, train_noise=NOISE, train_sampling=sp.asdict())
    assert s.trainer.train_sampling == sp and s.trainer.train_noise == NoiseModel(**NOISE)
    assert sum('sampled noisy MSE' in ln for ln in lines) == 1
    assert len(hist['loss_train']) == 2 and len(hist['loss_steps']) == 6 and all(np.isfinite(hist['loss_steps']))
    # the first step's loss is the sampled noisy loss of the header: the reference on the traced rows, stream seed + 1
    idx = np.asarray(hist['indices'][0])[:100]
    set_seed_model = _run(tmp_path, 'init', dev, num_epochs=0, train_noise=NOISE, train_sampling=sp)[0].model
    data = _solver_data()
    nz = NoiseModel(**NOISE, trajectories=8, seed=12)
    ref, _ = TG.model_loss_grad(set_seed_model.cpu(), (data['train_branch_input'][idx], data['train_trunk_input'][idx]),
                                data['train_output'][idx, 0], 1.0 / 100, TG.TrajEngine(nz, 0))
    assert abs(hist['loss_steps'][0] - ref[-2] / 100) < 1e-9
    # the ideal run differs; a run per step is the same run bitwise; so is a second run; another sampling seed is not
    _, ideal, _ = _run(tmp_path, 'ideal', dev)
    assert ideal['loss_steps'][0] != hist['loss_steps'][0]
    _, per_step, _ = _run(tmp_path, 'steps', dev, train_noise=NOISE, train_sampling=sp, epoch_call=False)
    assert per_step['loss_steps'] == hist['loss_steps']
    _, again, _ = _run(tmp_path, 'again', dev, train_noise=NOISE, train_sampling=sp)
    assert again['loss_steps'] == hist['loss_steps'] and again['loss_train'] == hist['loss_train']
    _, other, _ = _run(tmp_path, 'other', dev, train_noise=NOISE, train_sampling=Sampling(trajectories=8, seed=12))
    assert other['loss_steps'] != hist['loss_steps']
    # NoiseModel's own trajectories and seed stay ignored in training
    _, own, _ = _run(tmp_path, 'own', dev, train_noise=dict(NOISE, trajectories=3, seed=99), train_sampling=sp)
    assert own['loss_steps'] == hist['loss_steps']


@gpu
def test_solver_refusals(dev, tmp_path):
    from quanonet_amd.noise import DeviceNoise, Sampling
    from quanonet_amd.solver import PTSolver
    data = _solver_data()
    sp = Sampling(trajectories=4, seed=1)
    make = lambda name, **kw: PTSolver(_cfg(tmp_path, name, **kw), data, device=dev, log=quiet)
    with pytest.raises(ValueError, match='needs train_noise'):
        make('no_noise', train_sampling=sp)
    with pytest.raises(ValueError, match='train_device_noise'):
        make('device', train_device_noise=DeviceNoise(p1=0.01).asdict(), train_sampling=sp)
    with pytest.raises(ValueError, match='shots'):
        make('shots', train_noise=NOISE, train_sampling=Sampling(shots=100))
    for n in (6, 10):
        with pytest.raises(ValueError, match='7..9'):
            make(f'n{n}', train_noise=NOISE, train_sampling=sp, num_qubits=n)
    with pytest.raises(ValueError, match='Sampling'):
        make('type', train_noise=NOISE, train_sampling=8)
    with pytest.raises(ValueError, match='fused model-level path'):
        make('sgd', train_noise=NOISE, train_sampling=sp, optimizer='sgd')
    # without the key nothing changes: train_noise alone at n = 7 is refused as before
    with pytest.raises(ValueError, match='n <= 6'):
        make('alone', train_noise=NOISE)


def test_world_size_is_refused():
    """the trainer's own checks come before anything touches a device or a process group"""
    from quanonet_amd.noise import Sampling
    from quanonet_amd.solver import DataParallelTrainer
    m = torch.nn.Linear(2, 1).double()
    with pytest.raises(ValueError, match='world_size'):
        DataParallelTrainer(m, world_size=2, train_noise=NOISE, train_sampling=Sampling(trajectories=4))
    with pytest.raises(ValueError, match='needs train_noise'):
        DataParallelTrainer(m, train_sampling=Sampling(trajectories=4))
    with pytest.raises(ValueError, match='shots'):
        DataParallelTrainer(m, train_noise=NOISE, train_sampling={'shots': 5})
    with pytest.raises(ValueError, match='fused model-level path'):
        DataParallelTrainer(m, train_noise=NOISE, train_sampling=Sampling(trajectories=4))


def test_train_sampling_values():
    """the config value: a Sampling, its asdict() form, or nothing"""
    from quanonet_amd.solver import _train_sampling
    from quanonet_amd.noise import Sampling
    assert _train_sampling(None) is None
    assert _train_sampling({'trajectories': 4, 'seed': 2}) == Sampling(trajectories=4, seed=2)
    with pytest.raises(ValueError):
        _train_sampling({'trajectories': 0})


@gpu
def test_member_solvers_refuse_train_sampling(dev, tmp_path):
    from quanonet_amd.depth_sweep import DepthSweepSolver
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.qubit_sweep import QubitSweepSolver
    from quanonet_amd.sweep import SweepSolver
    data = _solver_data()
    for cls in (EnsembleSolver, SweepSolver, DepthSweepSolver, QubitSweepSolver):
        cfgs = [_cfg(tmp_path, cls.__name__, seed=k, run_id=f'm{k}', num_qubits=2) for k in (0, 1)]
        cfgs[1]['train_sampling'] = {'trajectories': 4}
        with pytest.raises(ValueError, match='train_sampling'):
            cls(cfgs, data, device=dev, log=quiet)
        cfgs[1]['train_noise'] = {'p1': 0.01}
        with pytest.raises(ValueError, match='train_noise'):
            cls(cfgs, data, device=dev, log=quiet)
