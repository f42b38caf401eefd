"""Seeded synthetic inputs of the critic / DDPG goldens (TEST INFRASTRUCTURE, own code).  tests/golden/gen_golden_ddpg.py
feeds them to the reference and the tests regenerate them from the stored seeds, checked against the stored checksums, so
the fixtures hold no (B,K,N,N) operators.

Critic inputs: states (B,1,n_s,N) ~ N(0,1), actions (B,1,n_a,N) ~ 0.5 N(0,1), gso (B,K,N,N) = I, A, A^2, ... of one
row-normalised random geometric graph per sample (oracle/synth.py), as MultiAgentStateWithDelay.curr_gso forms them.
A DDPG transition batch adds the delayed inputs (oracle/synth.make_inputs), rewards and notdone flags, for s and s'.
"""
import numpy as np

from oracle import synth


def gso_powers(rs, B, K, N):
    G = np.zeros((B, K, N, N), dtype=np.float32)
    for b in range(B):
        A = synth.geometric_adjacency(rs, N).astype(np.float32)
        G[b, 0] = np.eye(N, dtype=np.float32)
        for k in range(1, K):
            G[b, k] = A @ G[b, k - 1]
    return G


def critic_inputs(seed, B, K, N, n_s=6, n_a=2):
    rs = np.random.RandomState(seed)
    S = rs.randn(B, 1, n_s, N).astype(np.float32)
    A = (0.5 * rs.randn(B, 1, n_a, N)).astype(np.float32)
    G = gso_powers(rs, B, K, N)
    return S, A, G


def critic_affine(seed, hidden):
    """GroupNorm affine away from the default ones / zeros, so the tests see gamma and beta at work."""
    rs = np.random.RandomState(seed + 5)
    return [((1.0 + 0.2 * rs.randn(h)).astype(np.float32), (0.2 * rs.randn(h)).astype(np.float32)) for h in hidden]


def ddpg_batch(seed, B, K, N, n_s=6, n_a=2):
    """dict of numpy arrays: S, G, Xd, Gd (state), nS, nG, nXd, nGd (next state), A (B,1,n_a,N), r (B,), nd (B,)."""
    d = {}
    for pre, off in (('', 0), ('n', 1000)):
        S, _, G = critic_inputs(seed + off, B, K, N, n_s, n_a)
        Xd, Gd = synth.make_inputs(seed + off + 17, B, K, n_s, N)
        Xd[:, 0:1] = S
        d[pre + 'S'], d[pre + 'G'], d[pre + 'Xd'], d[pre + 'Gd'] = S, G, Xd, Gd
    rs = np.random.RandomState(seed + 2)
    d['A'] = np.clip(0.5 * rs.randn(B, 1, n_a, N), -1, 1).astype(np.float32)
    d['r'] = rs.randn(B).astype(np.float32)
    d['nd'] = (rs.uniform(size=B) > 0.2).astype(np.float32)
    return d


def batch_checksum(d):
    return synth.checksum(*[d[k] for k in sorted(d)])
