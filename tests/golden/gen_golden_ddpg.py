#!/usr/bin/env python3
"""Generate the critic / DDPG fixtures (tests/golden/critic_*.npz, ddpg_*.npz) by RUNNING THE REFERENCE ITSELF.

Run in the build container only (needs the reference tree, path in REF below):

    python tests/golden/gen_golden_ddpg.py

The reference cannot import its DDPG module as shipped; three shims, none of which changes a line of its source, make it
run on the CPU: a stub `gym` module in sys.modules, a neutral sys.argv for the module-level argparse, and
`learner.critic.F = torch.nn.functional` (critic.py calls F.relu without importing F).  Inputs come from
tests/ddpg_inputs.py (seeds + checksums are stored, never the operators); only arrays are written.
"""
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, REF)

sys.modules.setdefault('gym', types.ModuleType('gym'))
_argv, sys.argv = sys.argv, [sys.argv[0]]
import learner.critic as ref_critic  # noqa: E402
ref_critic.F = torch.nn.functional
from learner.critic import Critic as RefCritic  # noqa: E402
from learner import gnn_ddpg as ref_ddpg  # noqa: E402
from learner.replay_buffer import Transition as RefTransition  # noqa: E402
sys.argv = _argv

import ddpg_inputs as di  # noqa: E402

torch.set_num_threads(1)


def sd_to_np(sd, prefix):
    return {prefix + k.replace('.', '__'): v.detach().cpu().numpy().copy() for k, v in sd.items()}


def critic_init(seed, n_s, n_a, h, K):
    torch.manual_seed(seed)
    c = RefCritic(n_s, n_a, [h, h], K)
    d = dict(seed=seed, dims=np.array([n_s, n_a, h, K]))
    d.update(sd_to_np(c.state_dict(), 'w__'))
    path = os.path.join(HERE, 'critic_init_h%d_k%d.npz' % (h, K))
    np.savez_compressed(path, **d)
    print('wrote', path)


def critic_case(seed, B, N, K, h, n_s):
    torch.manual_seed(seed)
    c = RefCritic(n_s, 2, [h, h], K)
    with torch.no_grad():
        for norm, (g, b) in zip(c.layer_norms, di.critic_affine(seed, [h, h])):
            norm.weight.copy_(torch.from_numpy(g))
            norm.bias.copy_(torch.from_numpy(b))
    S, A, G = di.critic_inputs(seed, B, K, N, n_s)
    at = torch.from_numpy(A).requires_grad_(True)
    q = c(torch.from_numpy(S), at, torch.from_numpy(G))
    dQ = np.random.RandomState(seed + 3).randn(B, 1, N).astype(np.float32)
    q.backward(torch.from_numpy(dQ))
    d = dict(seed=seed, shape=np.array([B, N, K, h, n_s]), in_checksum=di.synth.checksum(S, A, G), dQ=dQ,
             Q=q.detach().numpy(), dA=at.grad.numpy())
    d.update(sd_to_np(c.state_dict(), 'w__'))
    for n, p in c.named_parameters():
        d['g__' + n.replace('.', '__')] = p.grad.numpy().copy()
    path = os.path.join(HERE, 'critic_fwd_B%d_N%d_K%d_h%d.npz' % (B, N, K, h))
    np.savez_compressed(path, **d)
    print('wrote', path, 'Q absmax', float(np.abs(d['Q']).max()))


def ref_batch(d, B, N, n_a=2):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    st = [SimpleNamespace(values=t(d['S'][b:b + 1]), curr_gso=t(d['G'][b:b + 1]), delay_state=t(d['Xd'][b:b + 1]),
                          delay_gso=t(d['Gd'][b:b + 1])) for b in range(B)]
    nx = [SimpleNamespace(values=t(d['nS'][b:b + 1]), curr_gso=t(d['nG'][b:b + 1]), delay_state=t(d['nXd'][b:b + 1]),
                          delay_gso=t(d['nGd'][b:b + 1])) for b in range(B)]
    return RefTransition(tuple(st), tuple(t(d['A'][b:b + 1]) for b in range(B)), tuple(t(d['nd'][b:b + 1]) for b in range(B)),
                         tuple(nx), tuple(t(d['r'][b:b + 1]) for b in range(B)))


def ddpg_case(seed, B, N, K, h):
    args = SimpleNamespace(n_states=6, n_actions=2, k=K, hidden_size=h, gamma=0.99, tau=0.5, n_agents=N)
    torch.manual_seed(seed)
    learner = ref_ddpg.DDPG(torch.device('cpu'), args)
    out = dict(seed=seed, shape=np.array([B, N, K, h]))
    for name in ('actor', 'actor_target', 'critic', 'critic_target'):
        out.update(sd_to_np(getattr(learner, name).state_dict(), 'init__%s__' % name))
    for step in range(2):
        d = di.ddpg_batch(seed + 100 * step, B, K, N)
        out['in_checksum_%d' % step] = di.batch_checksum(d)
        closs, ploss = learner.gradient_step(ref_batch(d, B, N))
        out['critic_loss_%d' % step], out['policy_loss_%d' % step] = np.float64(closs), np.float64(ploss)
        for name in ('actor', 'actor_target', 'critic', 'critic_target'):
            out.update(sd_to_np(getattr(learner, name).state_dict(), 's%d__%s__' % (step, name)))
    path = os.path.join(HERE, 'ddpg_step_B%d_N%d_K%d_h%d.npz' % (B, N, K, h))
    np.savez_compressed(path, **out)
    print('wrote', path, 'losses', [float(out[k]) for k in sorted(out) if 'loss' in k])


def ou_case(seed):
    np.random.seed(seed)
    ou = ref_ddpg.OUNoise(2, 5, scale=1)
    seq = [ou.noise() for _ in range(6)]
    ou.reset()
    seq += [ou.noise() for _ in range(2)]
    ou2 = ref_ddpg.OUNoise(2, 5)                      # default scale 0.05
    seq += [ou2.noise() for _ in range(2)]
    path = os.path.join(HERE, 'ddpg_ounoise.npz')
    np.savez_compressed(path, seed=seed, seq=np.stack(seq))
    print('wrote', path)


if __name__ == '__main__':
    critic_init(3, 6, 2, 32, 3)
    critic_init(8, 6, 2, 16, 1)
    for i, (B, N, K, h, n_s) in enumerate([(1, 16, 1, 16, 4), (5, 16, 3, 32, 6), (20, 100, 3, 32, 6), (8, 200, 4, 64, 6)]):
        critic_case(40 + i, B, N, K, h, n_s)
    ddpg_case(7, 5, 16, 3, 32)
    ddpg_case(9, 20, 100, 3, 32)
    ou_case(5)
