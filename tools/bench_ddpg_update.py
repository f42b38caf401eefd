#!/usr/bin/env python3
"""Time one DDPG update (learner/gnn_ddpg.py gradient_step after batch assembly): eager launches, the HIP-graph replay, and
the same update written in plain torch ATen ops (autograd + torch.optim.Adam) on the same GPU.  Prints one JSON record.

    python tools/bench_ddpg_update.py [--iters 200]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPES = [(20, 100, 3, 32), (100, 40, 1, 16)]      # (B, N, K, hidden)


def _time(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def _count_kernels(fn):
    try:
        from torch.profiler import profile, ProfilerActivity
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception:
        return None


def aten_update(d, B, N, K, h, gamma=0.99, tau=0.5):
    """The reference update in ATen ops on the device (restated, not imported): returns a closure doing one update."""
    F = torch.nn.functional
    torch.manual_seed(0)
    dev = torch.device('cuda')

    def actor_params():
        return [torch.nn.Parameter(torch.randn(s, device=dev) * 0.1) for s in
                [(h, 6, 1, 1), (h,), (h, h, K, 1), (h,), (2, h, 1, 1), (2,)]]

    def critic_params():
        ps = []
        for c_in, c_out in ((8, h), (h, h), (h, 1)):
            ps += [torch.nn.Parameter(torch.randn(c_out, K, c_in, 1, device=dev) * 0.1),
                   torch.nn.Parameter(torch.zeros(c_out, device=dev))]
        for _ in range(2):
            ps += [torch.nn.Parameter(torch.ones(h, device=dev)), torch.nn.Parameter(torch.zeros(h, device=dev))]
        return ps

    def actor(P, X, G):
        x = X.permute(0, 2, 1, 3)
        x = torch.tanh(F.conv2d(x, P[0], P[1]))
        x = torch.matmul(x.permute(0, 2, 1, 3), G).permute(0, 2, 1, 3)
        x = torch.tanh(F.conv2d(x, P[2], P[3], stride=(K, 1)))
        return F.conv2d(x, P[4], P[5]).view(B, 1, 2, N)

    def critic(P, S, A, G):
        x = torch.cat((S, A), 2)
        for i in range(3):
            W = P[2 * i]
            x = F.conv2d(torch.matmul(x, G), W, P[2 * i + 1], stride=(W.shape[2], 1))
            if i < 2:
                x = F.relu(F.group_norm(x, h, P[6 + 2 * i], P[7 + 2 * i], 1e-5))
            x = x.view(B, 1, W.shape[0], N)
        return x.view(B, 1, N)

    Pa, Pc = actor_params(), critic_params()
    Pat, Pct = [p.detach().clone() for p in Pa], [p.detach().clone() for p in Pc]
    oa, oc = torch.optim.Adam(Pa, lr=1e-5), torch.optim.Adam(Pc, lr=1e-4)
    t = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    r, nd = t['r'].view(B, 1), t['nd'].view(B, 1)

    def step():
        with torch.no_grad():
            qt = critic(Pct, t['nS'], actor(Pat, t['nXd'], t['nGd']), t['nG'])
            y = r + gamma * nd * qt
        oc.zero_grad()
        loss = ((critic(Pc, t['S'], t['A'], t['G']) - y) ** 2).mean()
        loss.backward()
        oc.step()
        oa.zero_grad()
        pl = -critic(Pc, t['S'], actor(Pa, t['Xd'], t['Gd']), t['G']).mean()
        pl.backward()
        oa.step()
        with torch.no_grad():
            for tp, p in zip(Pat + Pct, Pa + Pc):
                tp.copy_(tp * (1.0 - tau) + tau * p)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    a = ap.parse_args()
    import ddpg_inputs as di
    from test_gpu_ddpg import _batch, _learner
    from multiagent_gnn_policies_amd import ops
    rec = dict(metric='ddpg_update_us', device=torch.cuda.get_device_name(0), shapes=[])
    for B, N, K, h in SHAPES:
        d = di.ddpg_batch(1, B, K, N)
        batch = _batch(d, B)
        row = dict(B=B, N=N, K=K, hidden=h, critic_path='fused' if ops.critic_supported([8, h, h, 1], B, K, N) else 'composed')
        for graphed in (False, True):
            learner = _learner(1, N, K, h, graphed)
            learner.gradient_step(batch)
            u = learner.update_for(B, N)
            fn = (lambda u=u, g=graphed: u.run(g))
            row['graphed_us' if graphed else 'eager_us'] = round(_time(fn, a.iters), 2)
            if not graphed:
                row['launches_per_update'] = _count_kernels(fn)
        row['gradient_step_us'] = round(_time(lambda: learner.gradient_step(batch, sync=False), max(20, a.iters // 4)), 2)
        aten = aten_update(d, B, N, K, h)
        row['aten_us'] = round(_time(aten, a.iters), 2)
        row['aten_launches'] = _count_kernels(aten)
        rec['shapes'].append(row)
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
