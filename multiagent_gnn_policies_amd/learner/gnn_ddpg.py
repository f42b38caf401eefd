"""DDPG learner and training loop -- drop-in for reference learner/gnn_ddpg.py:36-377.

`OUNoise`, `DDPG(device, args)` (`hard_update` / `soft_update` / `select_action` / `gradient_step` / `save_model` /
`load_model`) and `train_ddpg(env, args, device)`.  The networks are an `Actor` with `ind_agg = 1` and the centralized
`Critic`, each with a target copy; the arithmetic of an update runs in the HIP kernels of libmgp.so: the actor on the
composed aggregation / dense kernels, the critic on mgp_critic_fwd / _bwd (or its composed path), the broadcast critic loss
and the policy loss on mgp_ddpg_*_loss, Adam on flat parameter buffers (mgp_adam_step_dev) and the target updates on
mgp_soft_update.  After the batch is assembled an update is a fixed sequence of launches on static buffers, captured once
per batch size as a HIP graph and replayed.

Deviations from the reference, each forced by what it cannot run as shipped or by the cfg-file interface of train.py:
  * `args` may be the reference's attribute namespace or a cfg section (train.py); the cfg supplies what the reference took
    from argparse, and `n_train_episodes` replaces its hard-coded `n_episodes = 10000`.
  * `train_ddpg` returns {'mean', 'std'} over `n_test_episodes` final noiseless episodes, as the other algorithms do; it
    prints progress and saves the networks only when `debug` (saving also needs `fname`).
  * `load_model` loads the state dicts onto the learner's device (the reference calls `.to()` on a dict, which raises).
"""
import os

import numpy as np
import torch

from .. import ops
from .actor import Actor
from .critic import Critic
from .gnn_dagger import FlatAdam
from .replay_buffer import ReplayBuffer, Transition
from .state_with_delay import MultiAgentStateWithDelay


class OUNoise:
    """Ornstein-Uhlenbeck exploration noise for the (N, nA) action array: each draw moves the process by
    theta (mu - x) + sigma * N(0, 1) (numpy's global stream) and returns the new state times `scale`."""

    def __init__(self, n_a, n_agents, scale=0.05, mu=0, theta=0.15, sigma=0.2):
        self.nA, self.n_agents = n_a, n_agents
        self.scale, self.mu, self.theta, self.sigma = scale, mu, theta, sigma
        self.reset()

    def reset(self):
        self.state = np.ones((self.n_agents, self.nA)) * self.mu

    def noise(self):
        x = self.state
        self.state = x + (self.theta * (self.mu - x) + self.sigma * np.random.standard_normal(np.shape(x)))
        return self.state * self.scale


def _arg(args, key, kind):
    """One setting from an attribute namespace (the reference's argparse) or a cfg section (train.py)."""
    if hasattr(args, 'getint'):
        return {int: args.getint, float: args.getfloat, str: args.get}[kind](key)
    return kind(getattr(args, key))


def _flatten(module):
    """Re-home every parameter of `module` as a view into one contiguous fp32 buffer (keys and shapes unchanged)."""
    params = list(module.parameters())
    flat = torch.empty((sum(p.numel() for p in params),), device=params[0].device, dtype=torch.float32)
    off = 0
    with torch.no_grad():
        for p in params:
            n = p.numel()
            flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = flat[off:off + n].view(p.shape)
            off += n
    return flat


# ------------------------------------------------------------------------------------ actor forward / backward without autograd
def _actor_forward(actor, X, G):
    """The Actor's composed forward (learner/actor.py) keeping what _actor_backward needs.  X (B,K,F,N) -> (B,nA,1,N)."""
    x = X.permute(0, 2, 1, 3)
    saved = []
    for i, conv in enumerate(actor.conv_layers):
        agg = i == actor.ind_agg
        if agg:
            x = ops.agg_fwd(x, G)
        out_c, in_c, step, _ = conv.weight.shape
        shape = tuple(x.shape)
        if step > 1:
            x = x.reshape(shape[0], in_c * step, 1, shape[3])
        act = ops.ACT_TANH if i < actor.n_layers - 1 else ops.ACT_NONE
        out = ops.dense_fwd(x, conv.weight.view(out_c, in_c * step), conv.bias, act)
        saved.append((x, out, agg, shape, act))
        x = out
    return x, saved


def _actor_backward(actor, saved, G, dOut):
    """Parameter gradients of the Actor in its parameter order (W0, b0, W1, b1, ...) from dOut (B,nA,1,N)."""
    grads = [None] * (2 * actor.n_layers)
    g = dOut
    for i in range(actor.n_layers - 1, -1, -1):
        inp, out, agg, shape, act = saved[i]
        conv = actor.conv_layers[i]
        out_c, in_c, step, _ = conv.weight.shape
        need = i > 0
        dW, db, dIn = ops.dense_bwd(g, out, inp, conv.weight.view(out_c, in_c * step), act, need)
        grads[2 * i], grads[2 * i + 1] = dW, db
        if not need:
            break
        dIn = dIn.view(shape)
        g = ops.agg_bwd_x(dIn, G) if agg else dIn
    return grads


class DDPGUpdate(object):
    """One DDPG update (reference gnn_ddpg.py:169-222) on static buffers for batch size B: target actor and critic forward on
    s' -> critic loss and dQ -> critic backward -> critic Adam -> actor forward -> critic forward and backward for dActions ->
    actor backward -> actor Adam -> both soft updates.  `run()` enqueues it eagerly, or (graphed) replays a HIP graph
    captured at the second call (the first call runs eagerly, so every one-time setup happens outside the capture)."""

    def __init__(self, learner, B, N):
        dev = learner.device
        a, c = learner.actor, learner.critic
        K, ns, na = a.k, learner.n_states, learner.n_actions
        f32 = dict(device=dev, dtype=torch.float32)
        self.S, self.nS = torch.empty((B, 1, ns, N), **f32), torch.empty((B, 1, ns, N), **f32)
        self.A = torch.empty((B, 1, na, N), **f32)
        self.G, self.nG = torch.empty((B, K, N, N), **f32), torch.empty((B, K, N, N), **f32)
        self.Xd, self.nXd = torch.empty((B, K, ns, N), **f32), torch.empty((B, K, ns, N), **f32)
        self.Gd, self.nGd = torch.empty((B, K, N, N), **f32), torch.empty((B, K, N, N), **f32)
        self.r, self.nd = torch.empty((B,), **f32), torch.empty((B,), **f32)
        self.closs, self.ploss = torch.zeros((1,), **f32), torch.zeros((1,), **f32)
        self.dQ, self.dQp = torch.empty((B, N), **f32), torch.empty((B, N), **f32)
        self.learner, self.B, self.N = learner, B, N
        self.graph, self.calls = None, 0
        self.launches = None

    def _enqueue(self):
        lr = self.learner
        B, N, na, ns = self.B, self.N, lr.n_actions, lr.n_states
        fused = lr.critic.use_fused
        copt, aopt = lr.critic_optim, lr.actor_optim
        with torch.no_grad():
            a_next, _ = _actor_forward(lr.actor_target, self.nXd, self.nGd)
            Qt, _ = ops.critic_forward(self.nS, a_next.view(B, 1, na, N), self.nG, *lr.critic_target.params(), save=False,
                                       fused=fused)
            Ws, bs, gammas, betas = lr.critic.params()
            Q, sv = ops.critic_forward(self.S, self.A, self.G, Ws, bs, gammas, betas, save=True, fused=fused)
            ops.ddpg_critic_loss(Q, Qt, self.r, self.nd, lr.gamma, loss=self.closs, dQ=self.dQ)
            dWs, dbs, dgs, dbes, _ = ops.critic_backward(self.dQ, self.G, sv, Ws, gammas, ns, True, False)
            torch.cat([t.reshape(-1) for pair in zip(dWs, dbs) for t in pair] + [t for pair in zip(dgs, dbes) for t in pair],
                      out=copt.flat_grad)
            ops.adam_step_dev(copt.flat, copt.flat_grad, copt.m, copt.v, copt.lr, copt.step_dev, *copt.betas, copt.eps)
            act, saved = _actor_forward(lr.actor, self.Xd, self.Gd)
            Qp, svp = ops.critic_forward(self.S, act.view(B, 1, na, N), self.G, Ws, bs, gammas, betas, save=True, fused=fused)
            ops.ddpg_policy_loss(Qp, loss=self.ploss, dQ=self.dQp)
            dAct = ops.critic_backward(self.dQp, self.G, svp, Ws, gammas, ns, False, True)[4]
            grads = _actor_backward(lr.actor, saved, self.Gd, dAct.view(B, na, 1, N))
            torch.cat([t.reshape(-1) for t in grads], out=aopt.flat_grad)
            ops.adam_step_dev(aopt.flat, aopt.flat_grad, aopt.m, aopt.v, aopt.lr, aopt.step_dev, *aopt.betas, aopt.eps)
            ops.soft_update(lr.actor_target_flat, aopt.flat, lr.tau)
            ops.soft_update(lr.critic_target_flat, copt.flat, lr.tau)

    def run(self, graphed):
        if not graphed or self.calls == 0:
            self._enqueue()
        else:
            if self.graph is None:
                torch.cuda.synchronize()
                self.graph = torch.cuda.CUDAGraph()
                with ops.graph_capture(self.graph):
                    self._enqueue()
            self.graph.replay()
        self.calls += 1
        self.learner.actor_optim.step_count += 1
        self.learner.critic_optim.step_count += 1


class DDPG(object):

    @staticmethod
    def hard_update(target, source):
        """Copy the parameters of `source` into `target` (reference gnn_ddpg.py:80-88)."""
        with torch.no_grad():
            for t, p in zip(target.parameters(), source.parameters()):
                t.data.copy_(p.data)

    @staticmethod
    def soft_update(target, source, tau):
        """target <- target (1 - tau) + tau source per parameter (mgp_soft_update; reference gnn_ddpg.py:90-100)."""
        for t, p in zip(target.parameters(), source.parameters()):
            ops.soft_update(t.data, p.data.contiguous(), tau)

    def __init__(self, device, args):
        n_s, n_a = _arg(args, 'n_states', int), _arg(args, 'n_actions', int)
        k, hidden_size = _arg(args, 'k', int), _arg(args, 'hidden_size', int)
        self.gamma, self.tau = _arg(args, 'gamma', float), _arg(args, 'tau', float)
        self.n_agents, self.n_states, self.n_actions = _arg(args, 'n_agents', int), n_s, n_a
        self.device = device
        hidden_layers = [hidden_size, hidden_size]
        ind_agg = int(len(hidden_layers) / 2)          # aggregate halfway
        # creation order of the reference (gnn_ddpg.py:130-133): the torch RNG is consumed identically
        self.actor = Actor(n_s, n_a, hidden_layers, k, ind_agg).to(self.device)
        self.actor_target = Actor(n_s, n_a, hidden_layers, k, ind_agg).to(self.device)
        self.critic = Critic(n_s, n_a, hidden_layers, k).to(self.device)
        self.critic_target = Critic(n_s, n_a, hidden_layers, k).to(self.device)
        # learning rates hard-coded by the reference (gnn_ddpg.py:135-136)
        self.actor_optim = FlatAdam(self.actor, lr=1e-5)
        self.critic_optim = FlatAdam(self.critic, lr=1e-4)
        self.actor_target_flat = _flatten(self.actor_target)
        self.critic_target_flat = _flatten(self.critic_target)
        DDPG.hard_update(self.actor_target, self.actor)
        DDPG.hard_update(self.critic_target, self.critic)
        self.use_graph = True
        self._updates = {}

    def select_action(self, state, action_noise=None):
        """Actor on the delayed state -> (N, nA) on the device, plus the noise if given, clamped to [-1, 1]
        (reference gnn_ddpg.py:146-167)."""
        with torch.no_grad():
            mu = self.actor(state.delay_state, state.delay_gso)
        mu = mu.permute(0, 1, 3, 2).reshape((self.n_agents, self.n_actions))
        if action_noise is not None:
            mu = mu + torch.Tensor(action_noise.noise()).to(self.device)
        return mu.clamp(-1, 1)

    def update_for(self, B, N):
        """The static-buffer update of batch size B (built on first use)."""
        u = self._updates.get((B, N))
        if u is None:
            u = self._updates[(B, N)] = DDPGUpdate(self, B, N)
        return u

    def gradient_step(self, batch, sync=True):
        """One update on a batch of transitions (reference gnn_ddpg.py:169-222): critic on the current values and operator
        powers, actor on the delayed ones.  Returns (critic_loss, policy_loss) as floats, or as (1,) device tensors with
        sync=False (no host wait)."""
        B = len(batch.state)
        N = batch.state[0].values.shape[3]
        u = self.update_for(B, N)
        torch.cat([s.values for s in batch.state], out=u.S)
        torch.cat([s.curr_gso for s in batch.state], out=u.G)
        torch.cat([s.delay_state for s in batch.state], out=u.Xd)
        torch.cat([s.delay_gso for s in batch.state], out=u.Gd)
        torch.cat([s.values for s in batch.next_state], out=u.nS)
        torch.cat([s.curr_gso for s in batch.next_state], out=u.nG)
        torch.cat([s.delay_state for s in batch.next_state], out=u.nXd)
        torch.cat([s.delay_gso for s in batch.next_state], out=u.nGd)
        torch.cat([a.reshape(1, 1, self.n_actions, N) for a in batch.action], out=u.A)
        torch.cat([r.reshape(1) for r in batch.reward], out=u.r)
        torch.cat([d.reshape(1) for d in batch.done], out=u.nd)
        u.run(self.use_graph)
        if not sync:
            return u.closs.clone(), u.ploss.clone()
        return u.closs.item(), u.ploss.item()

    def save_model(self, env_name, suffix="", actor_path=None, critic_path=None):
        """The reference's file names, typo included: models/ddpg_actor_<env>_<suffix>, models/dppg_critic_<env>_<suffix>."""
        if not os.path.exists('models/'):
            os.makedirs('models/')
        if actor_path is None:
            actor_path = "models/ddpg_actor_{}_{}".format(env_name, suffix)
        if critic_path is None:
            critic_path = "models/dppg_critic_{}_{}".format(env_name, suffix)
        print('Saving models to {} and {}'.format(actor_path, critic_path))
        torch.save({k: v.detach().clone() for k, v in self.actor.state_dict().items()}, actor_path)
        torch.save({k: v.detach().clone() for k, v in self.critic.state_dict().items()}, critic_path)

    def load_model(self, actor_path, critic_path):
        """Load state dicts onto the learner's device, in place (the flat-buffer views stay intact)."""
        print('Loading models from {} and {}'.format(actor_path, critic_path))
        for path, module in ((actor_path, self.actor), (critic_path, self.critic)):
            if path is None:
                continue
            sd = torch.load(path, map_location=self.device)
            own = module.state_dict()
            if set(sd) != set(own):
                raise KeyError("state_dict mismatch: unexpected %s, missing %s" % (sorted(set(sd) - set(own)),
                                                                                   sorted(set(own) - set(sd))))
            with torch.no_grad():
                for k_, v in sd.items():
                    own[k_].copy_(v)


def _episode(env, learner, args, device, noise=None, memory=None, on_step=None):
    """One episode; with `memory` every step files Transition(state, action, notdone, next_state, reward).  Returns the
    summed reward."""
    n_actions, n_agents = learner.n_actions, learner.n_agents
    state = MultiAgentStateWithDelay(device, args, env.reset(), prev_state=None)
    total, done = 0.0, False
    while not done:
        action = learner.select_action(state, noise)
        next_obs, reward, done, _ = env.step(action.cpu().numpy())
        next_state = MultiAgentStateWithDelay(device, args, next_obs, prev_state=state)
        total += reward
        if memory is not None:
            notdone = torch.Tensor([not done]).to(device)
            rew = torch.Tensor([reward]).to(device)
            action = action.transpose(1, 0).reshape((1, 1, n_actions, n_agents))
            memory.insert(Transition(state, action, notdone, next_state, rew))
        state = next_state
        if on_step is not None:
            on_step()
    return total


def train_ddpg(env, args, device):
    """Reference gnn_ddpg.py:307-377 on a cfg section: noisy training episodes, `updates_per_step` updates per environment
    step once the memory holds more than `batch_size` transitions, a noiseless evaluation episode after every 10th training
    episode, then `n_test_episodes` noiseless episodes whose mean and std are returned."""
    debug = bool(args.getboolean('debug')) if hasattr(args, 'getboolean') else bool(getattr(args, 'debug', False))
    fname = args.get('fname') if hasattr(args, 'get') else getattr(args, 'fname', None)
    batch_size, updates_per_step = _arg(args, 'batch_size', int), _arg(args, 'updates_per_step', int)
    memory = ReplayBuffer(max_size=_arg(args, 'buffer_size', int))
    learner = DDPG(device, args)
    ounoise = OUNoise(learner.n_actions, learner.n_agents, scale=1)
    rewards, counts = [], dict(steps=0, updates=0)

    def after_step():
        counts['steps'] += 1
        if memory.curr_size > batch_size:
            for _ in range(updates_per_step):
                batch = Transition(*zip(*memory.sample(batch_size)))
                learner.gradient_step(batch, sync=False)
                counts['updates'] += 1

    for i in range(_arg(args, 'n_train_episodes', int)):
        ounoise.reset()
        rewards.append(_episode(env, learner, args, device, ounoise, memory, after_step))
        if i % 10 == 0:
            rewards.append(_episode(env, learner, args, device))
            if debug:
                print("Episode: {}, updates: {}, total numsteps: {}, reward: {}, average reward: {}".format(
                    i, counts['updates'], counts['steps'], rewards[-1], np.mean(rewards[-10:])))
    test = [_episode(env, learner, args, device) for _ in range(_arg(args, 'n_test_episodes', int))]
    env.close()
    if debug and fname:
        learner.save_model(args.get('env') if hasattr(args, 'get') else args.env, suffix=fname)
    return {'mean': float(np.mean(test)), 'std': float(np.std(test))}
