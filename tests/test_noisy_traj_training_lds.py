"""
Sampled-trajectory noise-aware training at n = 10 through the Python layers: quanonet_amd.noise.sampled_noisy_loss_and_grad
against the numpy reference (and, at n = 8, bitwise against noisy_loss_and_grad), and DataParallelTrainer / PTSolver with
train_noise + train_trajectories (qhea_model_train_steps_noisy_lds at n >= 10, ..._noisy_wide below): the run, its
reproducibility, the per-step and the resumed path, the equality with train_sampling at n = 8, and every refusal.  What needs
no device is not marked gpu.
"""
import numpy as np
import pytest
import torch

from tests import noisy_traj_grad_reference as TG
from tests.test_noisy_forward import _solver_data
from tests.test_noisy_traj_grad_reference import build, inputs, noise_model
from tests.test_noisy_traj_training import NOISE, _cfg as _cfg7, quiet

gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _cfg(tmp_path, name, **kw):
    return _cfg7(tmp_path, name, **{'num_qubits': 10, **kw})


@gpu
def test_sampled_noisy_loss_and_grad(dev):
    from quanonet_amd.noise import DeviceNoise, NoiseModel, noisy_loss_and_grad, sampled_noisy_loss_and_grad
    for kind, readout in (('quanonet', 'X'), ('heaqnn', 'diag')):
        cpu = build(kind, 10, True, readout, seed=2)
        ins, y = inputs(kind, 4, seed=2), np.random.default_rng(2).normal(size=4)
        nz = noise_model((0.05, 0.1, 0.05), T=6, seed=21)
        ref, _ = TG.model_loss_grad(cpu, ins, y, 1.0 / 4, TG.TrajEngine(nz, 40))
        ref9, _ = TG.model_loss_grad(cpu, ins, y, 1.0 / 9, TG.TrajEngine(nz, 0))
        m = cpu.to(dev)
        dins = tuple(torch.tensor(t, device=dev) for t in ins)
        got = sampled_noisy_loss_and_grad(m, dins, torch.tensor(y, device=dev).reshape(-1, 1), nz, row0=40)
        got9 = sampled_noisy_loss_and_grad(m, dins, torch.tensor(y, device=dev), nz, inv_batch_total=1.0 / 9)
        torch.cuda.synchronize()
        print(f'{kind} {readout}: max|err| = {np.abs(got.cpu().numpy() - ref).max():.2e}, {np.abs(got9.cpu().numpy() - ref9).max():.2e}')
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=0, atol=1e-10)
        np.testing.assert_allclose(got9.cpu().numpy(), ref9, rtol=0, atol=1e-10)
    # at n = 8 it is noisy_loss_and_grad, bitwise
    m8 = build('quanonet', 8, True, 'Y', seed=3).to(dev)
    ins8 = tuple(torch.tensor(t, device=dev) for t in inputs('quanonet', 6, seed=3))
    y8 = torch.tensor(np.random.default_rng(3).normal(size=6), device=dev)
    nz = noise_model((0.05, 0.1, 0.05), T=9, seed=4)
    assert torch.equal(sampled_noisy_loss_and_grad(m8, ins8, y8, nz, row0=7), noisy_loss_and_grad(m8, ins8, y8, nz, row0=7))
    # refused inputs
    m = build('heaqnn', 10, True, 'Z').to(dev)
    x, y = (torch.tensor(inputs('heaqnn', 4)[0], device=dev),), torch.zeros(4, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match='shots'):
        sampled_noisy_loss_and_grad(m, x, y, NoiseModel(p1=0.01, shots=100))
    with pytest.raises(ValueError, match='DeviceNoise'):
        sampled_noisy_loss_and_grad(m, x, y, DeviceNoise(p1=0.01))
    with pytest.raises(ValueError, match='exact_noisy_loss_and_grad'):
        sampled_noisy_loss_and_grad(build('heaqnn', 6, True, 'Z').to(dev), x, y, NoiseModel(p1=0.01))
    with pytest.raises(TypeError):
        sampled_noisy_loss_and_grad(torch.nn.Linear(2, 1), x, y, NoiseModel(p1=0.01))
    assert sampled_noisy_loss_and_grad(m, (x[0][:0],), y[:0], NoiseModel(p1=0.01)).abs().sum().item() == 0.0  # an empty batch
    # noisy_loss_and_grad itself keeps its range
    with pytest.raises(ValueError, match='7..9'):
        noisy_loss_and_grad(m, x, y, NoiseModel(p1=0.01))


def _run(tmp_path, name, dev, seed=0, cfg=_cfg, **kw):
    from quanonet_amd.solver import PTSolver, set_random_seed
    set_random_seed(seed)
    lines = []
    s = PTSolver(cfg(tmp_path, name, **kw), _solver_data(), device=dev, log=lambda *a, **k: lines.append(' '.join(map(str, a))))
    return s, s.train(), lines


@gpu
def test_ptsolver_train_trajectories(dev, tmp_path):
    from quanonet_amd.noise import NoiseModel, Sampling
    sp = Sampling(trajectories=5, seed=11)                     # two full tiles and a tile of one
    s, hist, lines = _run(tmp_path, 'a', dev, train_noise=NOISE, train_trajectories=sp.asdict())
    assert s.trainer.train_sampling == sp and s.trainer.train_noise == NoiseModel(**NOISE)
    assert s.trainer.sampling_key == 'train_trajectories'
    assert sum('sampled noisy MSE' in ln for ln in lines) == 1
    assert len(hist['loss_train']) == 2 and len(hist['loss_steps']) == 6 and all(np.isfinite(hist['loss_steps']))
    # the first step's loss is the sampled noisy loss of the header: the reference on the traced rows, stream seed + 1
    idx = np.asarray(hist['indices'][0])[:100]
    init = _run(tmp_path, 'init', dev, num_epochs=0, train_noise=NOISE, train_trajectories=sp)[0].model
    data = _solver_data()
    nz = NoiseModel(**NOISE, trajectories=5, seed=12)
    ref, _ = TG.model_loss_grad(init.cpu(), (data['train_branch_input'][idx], data['train_trunk_input'][idx]),
                                data['train_output'][idx, 0], 1.0 / 100, TG.TrajEngine(nz, 0))
    print(f"first step: loss {hist['loss_steps'][0]:.12f}, reference {ref[-2] / 100:.12f}")
    assert abs(hist['loss_steps'][0] - ref[-2] / 100) < 1e-9
    # the ideal run differs; a run per step is the same run bitwise; so is a second run; another sampling seed is not
    _, ideal, _ = _run(tmp_path, 'ideal', dev)
    assert ideal['loss_steps'][0] != hist['loss_steps'][0]
    _, per_step, _ = _run(tmp_path, 'steps', dev, train_noise=NOISE, train_trajectories=sp, epoch_call=False)
    assert per_step['loss_steps'] == hist['loss_steps']
    _, again, _ = _run(tmp_path, 'again', dev, train_noise=NOISE, train_trajectories=sp)
    assert again['loss_steps'] == hist['loss_steps'] and again['loss_train'] == hist['loss_train']
    _, other, _ = _run(tmp_path, 'other', dev, train_noise=NOISE, train_trajectories=Sampling(trajectories=5, seed=12))
    assert other['loss_steps'] != hist['loss_steps']
    # NoiseModel's own trajectories and seed stay ignored in training
    _, own, _ = _run(tmp_path, 'own', dev, train_noise=dict(NOISE, trajectories=3, seed=99), train_trajectories=sp)
    assert own['loss_steps'] == hist['loss_steps']


@gpu
def test_a_resumed_trainer_continues_the_stream(dev):
    """three steps in one go, and two steps + a trainer that takes over parameters, moments and the Adam count: the third step
    draws from the stream keyed seed + 3 either way, so the runs agree bitwise"""
    from quanonet_amd.noise import Sampling
    from quanonet_amd.solver import DataParallelTrainer
    sp = Sampling(trajectories=5, seed=2 ** 64 - 2)            # seed + 3 wraps
    ins = tuple(torch.tensor(t, device=dev) for t in inputs('quanonet', 12, seed=1))
    y = torch.tensor(np.random.default_rng(1).normal(size=12), device=dev)
    batch = lambda i: (ins[0][4 * i:4 * i + 4], ins[1][4 * i:4 * i + 4], y[4 * i:4 * i + 4])
    make = lambda: DataParallelTrainer(build('quanonet', 10, True, 'Z', seed=6).to(dev), lr=2e-2, train_noise=NOISE,
                                       train_trajectories=sp)
    whole = make()
    for i in range(3):
        whole.train_step(*batch(i), row0=4 * i)
    first = make()
    for i in range(2):
        first.train_step(*batch(i), row0=4 * i)
    resumed = make()
    resumed.pflat.copy_(first.pflat)
    resumed.optimizer.exp_avg.copy_(first.optimizer.exp_avg)
    resumed.optimizer.exp_avg_sq.copy_(first.optimizer.exp_avg_sq)
    resumed.optimizer.t = first.optimizer.t
    out = resumed.train_step(*batch(2), row0=8)
    torch.cuda.synchronize()
    assert resumed.optimizer.t == 3
    assert torch.equal(resumed.pflat, whole.pflat) and torch.equal(out, whole._last)
    assert not torch.equal(first.pflat, whole.pflat)


@gpu
def test_train_trajectories_is_train_sampling_at_n8(dev, tmp_path):
    from quanonet_amd.noise import Sampling
    sp = Sampling(trajectories=5, seed=3)
    a = _run(tmp_path, 'sampling', dev, cfg=_cfg7, num_qubits=8, train_noise=NOISE, train_sampling=sp)
    b = _run(tmp_path, 'trajectories', dev, cfg=_cfg7, num_qubits=8, train_noise=NOISE, train_trajectories=sp)
    assert a[1]['loss_steps'] == b[1]['loss_steps'] and a[1]['loss_train'] == b[1]['loss_train']
    for pa, pb in zip(a[0].model.parameters(), b[0].model.parameters()):
        assert torch.equal(pa, pb)


@gpu
def test_solver_refusals(dev, tmp_path):
    from quanonet_amd.noise import DeviceNoise, Sampling
    from quanonet_amd.solver import PTSolver
    data = _solver_data()
    sp = Sampling(trajectories=4, seed=1)
    make = lambda name, **kw: PTSolver(_cfg(tmp_path, name, **kw), data, device=dev, log=quiet)
    with pytest.raises(ValueError, match='set one of them'):
        make('both', train_noise=NOISE, train_sampling=sp, train_trajectories=sp)
    with pytest.raises(ValueError, match='train_trajectories needs train_noise'):
        make('no_noise', train_trajectories=sp)
    with pytest.raises(ValueError, match='train_device_noise'):
        make('device', train_device_noise=DeviceNoise(p1=0.01).asdict(), train_trajectories=sp)
    with pytest.raises(ValueError, match='shots'):
        make('shots', train_noise=NOISE, train_trajectories=Sampling(shots=100))
    with pytest.raises(ValueError, match='7..12'):
        make('n6', train_noise=NOISE, train_trajectories=sp, num_qubits=6)
    with pytest.raises(ValueError, match='Sampling'):
        make('type', train_noise=NOISE, train_trajectories=8)
    with pytest.raises(ValueError, match='fused model-level path'):
        make('sgd', train_noise=NOISE, train_trajectories=sp, optimizer='sgd')
    # train_sampling keeps its range
    with pytest.raises(ValueError, match='7..9'):
        make('old', train_noise=NOISE, train_sampling=sp)


def test_what_needs_no_device():
    """the trainer's own checks come before anything touches a device or a process group"""
    from quanonet_amd.noise import Sampling
    from quanonet_amd.solver import DataParallelTrainer
    m = torch.nn.Linear(2, 1).double()
    sp = Sampling(trajectories=4)
    with pytest.raises(ValueError, match='world_size'):
        DataParallelTrainer(m, world_size=2, train_noise=NOISE, train_trajectories=sp)
    with pytest.raises(ValueError, match='set one of them'):
        DataParallelTrainer(m, train_noise=NOISE, train_sampling=sp, train_trajectories=sp)
    with pytest.raises(ValueError, match='train_trajectories needs train_noise'):
        DataParallelTrainer(m, train_trajectories=sp)
    with pytest.raises(ValueError, match='shots'):
        DataParallelTrainer(m, train_noise=NOISE, train_trajectories={'shots': 5})
    with pytest.raises(ValueError, match='train_trajectories needs the fused model-level path'):
        DataParallelTrainer(m, train_noise=NOISE, train_trajectories=sp)


@gpu
def test_member_solvers_refuse_train_trajectories(dev, tmp_path):
    from quanonet_amd.depth_sweep import DepthSweepSolver
    from quanonet_amd.ensemble import EnsembleSolver
    from quanonet_amd.qubit_sweep import QubitSweepSolver
    from quanonet_amd.sweep import SweepSolver
    data = _solver_data()
    for cls in (EnsembleSolver, SweepSolver, DepthSweepSolver, QubitSweepSolver):
        cfgs = [_cfg7(tmp_path, cls.__name__, seed=k, run_id=f'm{k}', num_qubits=2) for k in (0, 1)]
        cfgs[1]['train_trajectories'] = {'trajectories': 4}
        with pytest.raises(ValueError, match='train_trajectories'):
            cls(cfgs, data, device=dev, log=quiet)
