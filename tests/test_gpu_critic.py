"""The critic kernels on the MI355X: forward against the reference's outputs (tests/golden/critic_fwd_*.npz), backward
against an fp64 torch-autograd evaluation of the critic restated below, both the one-launch and the composed path, and
bit-identical repeat calls."""
import numpy as np
import pytest
import torch

from conftest import check_parity, load_golden
import ddpg_inputs as di

pytestmark = pytest.mark.gpu

CRITIC_GOLDENS = ['critic_fwd_B1_N16_K1_h16', 'critic_fwd_B5_N16_K3_h32', 'critic_fwd_B20_N100_K3_h32',
                  'critic_fwd_B8_N200_K4_h64']


def torch_critic(S, A, G, Ws, bs, gs, bes):
    """reference critic.py:69-85 in plain torch ops, any dtype / device."""
    F = torch.nn.functional
    B, N = S.shape[0], S.shape[3]
    x = torch.cat((S, A), 2)
    for i, (W, b) in enumerate(zip(Ws, bs)):
        x = F.conv2d(torch.matmul(x, G), W, b, stride=(W.shape[2], 1))
        if i < len(Ws) - 1:
            x = F.relu(F.group_norm(x, W.shape[0], gs[i], bes[i], 1e-5))
        x = x.view(B, 1, W.shape[0], N)
    return x.view(B, 1, N)


def _load(name, dev):
    g = load_golden(name)
    B, N, K, h, n_s = [int(v) for v in g['shape']]
    S, A, G = di.critic_inputs(int(g['seed']), B, K, N, n_s)
    assert abs(di.synth.checksum(S, A, G) - float(g['in_checksum'])) <= 1e-9 * max(1.0, abs(float(g['in_checksum'])))
    from multiagent_gnn_policies_amd.learner.critic import Critic
    c = Critic(n_s, 2, [h, h], K).to(dev)
    c.load_state_dict({k[3:].replace('__', '.'): torch.from_numpy(v) for k, v in g.items() if k.startswith('w__')})
    return g, c, (S, A, G)


def _witness(c, S, A, G, dQ):
    """fp64 evaluation of the restated critic and the distance of its fp32 evaluation from it (forward and gradients)."""
    out = {}
    for dt in (torch.float64, torch.float32):
        P = [p.detach().cpu().to(dt).requires_grad_(True) for p in c.parameters()]
        nl = c.n_layers
        Ws, bs, gs, bes = P[0:2 * nl:2], P[1:2 * nl:2], P[2 * nl::2], P[2 * nl + 1::2]
        a = torch.from_numpy(A).to(dt).requires_grad_(True)
        q = torch_critic(torch.from_numpy(S).to(dt), a, torch.from_numpy(G).to(dt), Ws, bs, gs, bes)
        q.backward(torch.from_numpy(dQ).to(dt))
        out[dt] = [q.detach().double().numpy(), a.grad.double().numpy()] + [p.grad.double().numpy() for p in P]
    ref, f32 = out[torch.float64], out[torch.float32]
    noise = [float(np.max(np.abs(x - r) / np.maximum(1.0, np.abs(r).max()))) for x, r in zip(f32, ref)]
    return ref, noise


@pytest.mark.parametrize('name', CRITIC_GOLDENS)
@pytest.mark.parametrize('fused', [True, False])
def test_critic_forward_and_backward(name, fused):
    from multiagent_gnn_policies_amd import ops
    dev = torch.device('cuda')
    g, c, (S, A, G) = _load(name, dev)
    B, N, K, h, n_s = [int(v) for v in g['shape']]
    c.use_fused = fused
    path = 'fused' if fused and ops.critic_supported(c.layers, B, K, N) else 'composed'
    print('%s: %s path' % (name, path))
    if fused:
        assert (path == 'fused') == (name != 'critic_fwd_B8_N200_K4_h64'), "coverage changed for %s" % name
    a = torch.from_numpy(A).to(dev).requires_grad_(True)
    q = c(torch.from_numpy(S).to(dev), a, torch.from_numpy(G).to(dev))
    dQ = g['dQ']
    q.backward(torch.from_numpy(dQ).to(dev))
    ref, noise = _witness(c, S, A, G, dQ)
    # forward against the reference's own output: plain bound, or within its fp32 scatter where GroupNorm amplifies
    check_parity(q.detach().cpu().numpy(), g['Q'], noise[0], '%s Q (%s)' % (name, path))
    check_parity(q.detach().cpu().numpy(), ref[0], noise[0], '%s Q vs fp64 (%s)' % (name, path))
    got = [a.grad.cpu().numpy()] + [p.grad.cpu().numpy() for p in c.parameters()]
    names = ['dActions'] + [n for n, _ in c.named_parameters()]
    for x, r, nz, n in zip(got, ref[1:], noise[1:], names):
        scale = max(1.0, float(np.abs(r).max()))
        err = float(np.max(np.abs(x - r))) / scale
        assert err <= 1e-5 + 2.0 * nz, (name, path, n, err, nz)


@pytest.mark.parametrize('name', ['critic_fwd_B20_N100_K3_h32', 'critic_fwd_B8_N200_K4_h64'])
def test_critic_repeat_calls_are_bit_identical(name):
    from multiagent_gnn_policies_amd import ops
    dev = torch.device('cuda')
    g, c, (S, A, G) = _load(name, dev)
    S, A, G = (torch.from_numpy(x).to(dev) for x in (S, A, G))
    dQ = torch.from_numpy(g['dQ']).to(dev).view(S.shape[0], -1)
    Ws, bs, gs, bes = c.params()
    outs = []
    for _ in range(2):
        Q, sv = ops.critic_forward(S, A, G, [w.detach() for w in Ws], [b.detach() for b in bs], [x.detach() for x in gs],
                                   [x.detach() for x in bes])
        dWs, dbs, dgs, dbes, dAct = ops.critic_backward(dQ, G, sv, [w.detach() for w in Ws], [x.detach() for x in gs],
                                                        c.n_s, True, True)
        outs.append([Q] + dWs + dbs + dgs + dbes + [dAct])
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_ddpg_losses_match_torch():
    """mgp_ddpg_critic_loss against F.mse_loss on the reference's (B,1,N) - (B,B,N) broadcast, and the policy loss."""
    from multiagent_gnn_policies_amd import ops
    dev = torch.device('cuda')
    rs = np.random.RandomState(4)
    B, N = 7, 33
    Q = torch.from_numpy(rs.randn(B, N)).to(dev, torch.float32)
    Qt = torch.from_numpy(rs.randn(B, N)).to(dev, torch.float32)
    r = torch.from_numpy(rs.randn(B)).to(dev, torch.float32)
    nd = torch.tensor([1, 0, 1, 1, 1, 0, 1], dtype=torch.float32, device=dev)
    loss, dQ = ops.ddpg_critic_loss(Q, Qt, r, nd, 0.99)
    q = Q.double().view(B, 1, N).requires_grad_(True)
    y = r.double().view(B, 1) + (0.99 * nd.double().view(B, 1)) * Qt.double().view(B, 1, N)       # (B,B,N), as gnn_ddpg.py:195
    assert y.shape == (B, B, N)
    with pytest.warns(UserWarning):
        ref = torch.nn.functional.mse_loss(q, y)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-6 * max(1.0, abs(ref.item()))
    assert torch.allclose(dQ.double(), q.grad.view(B, N), rtol=1e-5, atol=1e-9)
    pl, dQp = ops.ddpg_policy_loss(Q)
    assert abs(pl.item() + Q.double().mean().item()) <= 1e-6
    assert torch.all(dQp == -1.0 / (B * N))
