"""Host-side checks of the critic / DDPG layer (no GPU): module layout and seeded initialisation against the reference's
own (tests/golden/gen_golden_ddpg.py), OU noise draws, cfg acceptance and the kernels' host-side coverage queries."""
import configparser
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


def _critic(seed, n_s, n_a, h, K):
    from multiagent_gnn_policies_amd.learner.critic import Critic
    torch.manual_seed(seed)
    return Critic(n_s, n_a, [h, h], K)


@pytest.mark.parametrize('name', ['critic_init_h32_k3', 'critic_init_h16_k1'])
def test_critic_default_init_is_the_reference_init(name):
    g = load_golden(name)
    n_s, n_a, h, K = [int(v) for v in g['dims']]
    c = _critic(int(g['seed']), n_s, n_a, h, K)
    sd = c.state_dict()
    assert sorted('w__' + k.replace('.', '__') for k in sd) == sorted(k for k in g if k.startswith('w__'))
    for k, v in sd.items():
        ref = g['w__' + k.replace('.', '__')]
        assert tuple(v.shape) == ref.shape, k
        assert np.array_equal(v.numpy(), ref), k


def test_critic_attributes_and_layout():
    c = _critic(0, 6, 2, 32, 3)
    assert c.layers == [8, 32, 32, 1] and c.n_layers == 3 and c.gso_first is True
    assert [tuple(m.weight.shape) for m in c.conv_layers] == [(32, 3, 8, 1), (32, 3, 32, 1), (1, 3, 32, 1)]
    assert [m.num_groups for m in c.layer_norms] == [32, 32] and all(m.eps == 1e-5 for m in c.layer_norms)
    names = [n for n, _ in c.named_parameters()]
    assert names[:6] == ['conv_layers.%d.%s' % (i, w) for i in range(3) for w in ('weight', 'bias')]
    assert names[6:] == ['layer_norms.%d.%s' % (i, w) for i in range(2) for w in ('weight', 'bias')]


@pytest.mark.parametrize('bad', ['batch_actions', 'batch_gso', 'state_plane', 'n_a', 'agents_actions', 'n_s', 'k',
                                 'gso_rows', 'gso_cols'])
def test_critic_assertions(bad):
    c = _critic(0, 6, 2, 16, 3)
    B, N = 2, 5
    shp = dict(s=[B, 1, 6, N], a=[B, 1, 2, N], g=[B, 3, N, N])
    edit = {'batch_actions': ('a', 0), 'batch_gso': ('g', 0), 'state_plane': ('s', 1), 'n_a': ('a', 2),
            'agents_actions': ('a', 3), 'n_s': ('s', 2), 'k': ('g', 1), 'gso_rows': ('g', 2), 'gso_cols': ('g', 3)}[bad]
    shp[edit[0]][edit[1]] += 1
    with pytest.raises(AssertionError):
        c(torch.zeros(shp['s']), torch.zeros(shp['a']), torch.zeros(shp['g']))


def test_ounoise_draws_equal_the_reference():
    from multiagent_gnn_policies_amd.learner.gnn_ddpg import OUNoise
    g = load_golden('ddpg_ounoise')
    np.random.seed(int(g['seed']))
    ou = OUNoise(2, 5, scale=1)
    seq = [ou.noise() for _ in range(6)]
    ou.reset()
    seq += [ou.noise() for _ in range(2)]
    ou2 = OUNoise(2, 5)
    seq += [ou2.noise() for _ in range(2)]
    assert np.array_equal(np.stack(seq), g['seq'])


@pytest.mark.parametrize('name', ['ddpg_step_B5_N16_K3_h32', 'ddpg_step_B20_N100_K3_h32'])
def test_ddpg_networks_are_built_in_the_reference_order(name):
    """actor, actor_target, critic, critic_target from one seed: the same four initialisations (then hard_update)."""
    from multiagent_gnn_policies_amd.learner.gnn_ddpg import DDPG
    g = load_golden(name)
    B, N, K, h = [int(v) for v in g['shape']]
    torch.manual_seed(int(g['seed']))
    learner = DDPG(torch.device('cpu'), SimpleNamespace(n_states=6, n_actions=2, k=K, hidden_size=h, gamma=0.99, tau=0.5,
                                                        n_agents=N))
    assert learner.actor.ind_agg == 1
    for net in ('actor', 'actor_target', 'critic', 'critic_target'):
        for k, v in getattr(learner, net).state_dict().items():
            assert np.array_equal(v.numpy(), g['init__%s__%s' % (net, k.replace('.', '__'))]), (net, k)


def test_check_experiment_accepts_ddpg():
    import train
    cp = configparser.ConfigParser()
    cp.read(os.path.join(ROOT, 'cfg', 'flocking_ddpg_n40_k1.cfg'))
    assert train.ALGORITHMS['ddpg'] is not None
    for name in cp.sections():
        assert cp[name].get('alg') == 'ddpg'
        train.check_experiment(cp[name])


def test_critic_coverage_query_needs_no_device():
    """One-launch coverage for the DDPG shapes the cfg files give (hidden 4..128, K 1..4, N <= 200) where the LDS plan fits;
    the rest run on the composed kernels."""
    from multiagent_gnn_policies_amd import ops
    assert ops.critic_supported([8, 32, 32, 1], 20, 3, 100)
    assert ops.critic_supported([8, 16, 16, 1], 100, 1, 40)
    assert ops.critic_supported([8, 4, 4, 1], 100, 4, 200)
    assert not ops.critic_supported([8, 64, 64, 1], 8, 4, 200)        # (3 * 64 + 64) * 200 floats > 160 KiB
    assert not ops.critic_supported([8, 128, 128, 1], 20, 3, 100)
    assert not ops.critic_supported([8, 32, 32, 2], 20, 3, 100)       # the critic ends in one channel
