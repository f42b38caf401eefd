"""DDPG on the MI355X: two consecutive gradient steps against the reference's own (tests/golden/ddpg_step_*.npz), graphed
replay against eager calls, the soft update against torch's op sequence, select_action, and short end-to-end runs."""
import configparser
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import ddpg_inputs as di

pytestmark = pytest.mark.gpu

NETS = ('actor', 'actor_target', 'critic', 'critic_target')


def _learner(seed, N, K, h, graphed=True):
    from multiagent_gnn_policies_amd.learner.gnn_ddpg import DDPG
    torch.manual_seed(seed)
    learner = DDPG(torch.device('cuda'), SimpleNamespace(n_states=6, n_actions=2, k=K, hidden_size=h, gamma=0.99, tau=0.5,
                                                         n_agents=N))
    learner.use_graph = graphed
    return learner


def _batch(d, B):
    from multiagent_gnn_policies_amd.learner.replay_buffer import Transition
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    st = [SimpleNamespace(values=t(d['S'][b:b + 1]), curr_gso=t(d['G'][b:b + 1]), delay_state=t(d['Xd'][b:b + 1]),
                          delay_gso=t(d['Gd'][b:b + 1])) for b in range(B)]
    nx = [SimpleNamespace(values=t(d['nS'][b:b + 1]), curr_gso=t(d['nG'][b:b + 1]), delay_state=t(d['nXd'][b:b + 1]),
                          delay_gso=t(d['nGd'][b:b + 1])) for b in range(B)]
    return Transition(tuple(st), tuple(t(d['A'][b:b + 1]) for b in range(B)), tuple(t(d['nd'][b:b + 1]) for b in range(B)),
                      tuple(nx), tuple(t(d['r'][b:b + 1]) for b in range(B)))


def _structural_zero(net, key, learner):
    """Conv biases in front of a GroupNorm: their gradient is zero in exact arithmetic (the norm removes every per-channel
    shift), so both sides feed Adam pure rounding noise, which it scales to steps of up to lr = 1e-4 in either direction:
    the two sides can part by 2 lr per step.  (Those biases cannot change any output.)"""
    if not net.startswith('critic') or not key.startswith('conv_layers.') or not key.endswith('.bias'):
        return False
    return int(key.split('.')[1]) < learner.critic.n_layers - 1


@pytest.mark.parametrize('name', ['ddpg_step_B5_N16_K3_h32', 'ddpg_step_B20_N100_K3_h32'])
def test_gradient_step_matches_reference(name):
    g = load_golden(name)
    B, N, K, h = [int(v) for v in g['shape']]
    seed = int(g['seed'])
    learner = _learner(seed, N, K, h)
    for step in range(2):
        d = di.ddpg_batch(seed + 100 * step, B, K, N)
        assert abs(di.batch_checksum(d) - float(g['in_checksum_%d' % step])) <= 1e-9 * abs(float(g['in_checksum_%d' % step]))
        closs, ploss = learner.gradient_step(_batch(d, B))
        for got, key in ((closs, 'critic_loss_%d' % step), (ploss, 'policy_loss_%d' % step)):
            ref = float(g[key])
            assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref)), (key, got, ref)
        for net in NETS:
            for k, v in getattr(learner, net).state_dict().items():
                ref = g['s%d__%s__%s' % (step, net, k.replace('.', '__'))]
                err = float(np.max(np.abs(v.cpu().numpy() - ref)))
                bound = 2e-4 * (step + 1) + 2e-6 if _structural_zero(net, k, learner) else 2e-6
                assert err <= bound, (name, step, net, k, err)


def test_graphed_replay_equals_eager_calls():
    B, N, K, h = 6, 24, 3, 16
    runs = []
    for graphed in (False, True):
        learner = _learner(21, N, K, h, graphed)
        losses = [learner.gradient_step(_batch(di.ddpg_batch(300 + s, B, K, N), B)) for s in range(4)]
        runs.append((losses, [torch.cat([p.detach().reshape(-1) for p in getattr(learner, n).parameters()]) for n in NETS]))
        if graphed:
            assert learner.update_for(B, N).graph is not None
    (l0, w0), (l1, w1) = runs
    assert l0 == l1
    for a, b in zip(w0, w1):
        assert torch.equal(a, b)


@pytest.mark.parametrize('tau', [0.5, 0.001, 0.3, 0.9])
def test_soft_update_is_torchs_op_sequence(tau):
    from multiagent_gnn_policies_amd import ops
    rs = np.random.RandomState(int(tau * 1000))
    t = torch.from_numpy(rs.randn(5000).astype(np.float32)).cuda()
    p = torch.from_numpy(rs.randn(5000).astype(np.float32)).cuda()
    ref = t * (1.0 - tau) + tau * p
    ops.soft_update(t, p, tau)
    assert torch.equal(t, ref)


def test_select_action_adds_noise_and_clamps():
    from multiagent_gnn_policies_amd.learner.gnn_ddpg import OUNoise
    N, K = 16, 3
    learner = _learner(2, N, K, 16)
    with torch.no_grad():
        learner.actor.conv_layers[2].bias.fill_(0.9)            # push some actions past the clamp
    d = di.ddpg_batch(5, 1, K, N)
    state = SimpleNamespace(delay_state=torch.from_numpy(d['Xd']).cuda(), delay_gso=torch.from_numpy(d['Gd']).cuda())
    with torch.no_grad():
        mu = learner.actor(state.delay_state, state.delay_gso).permute(0, 1, 3, 2).reshape(N, 2)
    np.random.seed(3)
    ou = OUNoise(2, N, scale=1)
    a = learner.select_action(state, ou)
    np.random.seed(3)
    ou_ref = OUNoise(2, N, scale=1)
    expect = (mu + torch.Tensor(ou_ref.noise()).cuda()).clamp(-1, 1)
    assert torch.equal(a, expect) and a.shape == (N, 2)
    assert float(a.abs().max()) <= 1.0 and bool((a.abs() == 1.0).any())
    assert torch.equal(learner.select_action(state), mu.clamp(-1, 1))


def _tiny_cfg():
    cp = configparser.ConfigParser()
    cp['DEFAULT'] = dict(header='alg, reward', debug='False', seed='3', env='FlockingRelative-v0', n_agents='16',
                         n_states='6', n_actions='2', comm_radius='1.0', v_max='3.0', dt='0.01', centralized='False',
                         k='3', hidden_size='16', n_train_episodes='2', n_test_episodes='2', test_interval='1',
                         updates_per_step='1', batch_size='8', buffer_size='1000', gamma='0.99', tau='0.5', actor_lr='1e-5',
                         beta_coeff='0.993')
    cp['ddpg'] = dict(alg='ddpg')
    return cp


def test_train_ddpg_short_run():
    import train
    stats = train.run_experiment(_tiny_cfg()['ddpg'])
    assert set(stats) == {'mean', 'std'} and np.isfinite(stats['mean']) and np.isfinite(stats['std'])


def test_train_py_runs_a_ddpg_cfg(tmp_path):
    path = tmp_path / 'ddpg_tiny.cfg'
    with open(path, 'w') as f:
        _tiny_cfg().write(f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), str(path)], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[0] == 'alg, reward' and lines[-1].startswith('ddpg, ')
    assert all(np.isfinite(float(x)) for x in lines[-1].split(', ')[1:])
