"""`Critic` -- drop-in for the reference's centralized Q-network (reference learner/critic.py:7-87).

Same constructor `(n_s, n_a, hidden_layers, k)`, attributes (`layers`, `n_layers`, `gso_first`, `conv_layers`,
`layer_norms`), `state_dict` keys and shapes (`conv_layers.{i}.weight (out, K, C_in, 1)` / `.bias`,
`layer_norms.{i}.weight / .bias`), assertion behaviour, and creation order (convs, then norms), so a seeded default
initialisation consumes the torch RNG exactly like the reference.  The modules only hold parameters: the forward and its
backward are the HIP kernels of libmgp.so (ops.critic: one launch per direction where mgp_critic_supported covers the
shape, else the composed aggregation / dense / GroupNorm+ReLU kernels).  Every layer is GSO -> filter -> GroupNorm ->
ReLU; the last layer stops after the filter.
"""
import numpy as np
import torch.nn as nn

from .. import ops


class Critic(nn.Module):

    def __init__(self, n_s, n_a, hidden_layers, k):
        """n_s features and n_a action axes per agent; `hidden_layers` lists the hidden widths; `k` graph-shift taps."""
        super().__init__()
        self.k, self.n_s, self.n_a = k, n_s, n_a
        self.layers = [n_s + n_a] + list(hidden_layers) + [1]
        self.n_layers = len(self.layers) - 1
        self.gso_first = True
        # every layer sees the K tap planes as its Conv2d channels and one layer's width as its kernel height
        self.conv_layers = nn.ModuleList([
            nn.Conv2d(k, c_out, kernel_size=(c_in, 1), stride=(c_in, 1))
            for c_in, c_out in zip(self.layers[:-1], self.layers[1:])])
        self.layer_norms = nn.ModuleList([nn.GroupNorm(c, c) for c in self.layers[1:-1]])
        self.use_fused = True       # one-launch kernels where the shape is covered (ops.critic_supported)

    def _check_shapes(self, states, actions, gso):
        """AssertionError on every mismatch the reference asserts (critic.py:58-67)."""
        batch_size = np.shape(states)[0]
        n_agents = states.shape[3]
        assert batch_size == actions.shape[0]
        assert batch_size == gso.shape[0]
        assert states.shape[1] == 1
        assert actions.shape[2] == self.n_a
        assert actions.shape[3] == n_agents
        assert states.shape[2] == self.n_s
        assert gso.shape[1] == self.k
        assert gso.shape[2] == n_agents
        assert gso.shape[3] == n_agents
        return batch_size, n_agents

    def params(self):
        """(Ws, bs, gammas, betas) in layer order."""
        return ([c.weight for c in self.conv_layers], [c.bias for c in self.conv_layers],
                [n.weight for n in self.layer_norms], [n.bias for n in self.layer_norms])

    def forward(self, states, actions, gso):
        """states (B,1,n_s,N), actions (B,1,n_a,N), gso (B,K,N,N) = [I, A, A^2, ...]  ->  Q (B,1,N)."""
        batch_size, n_agents = self._check_shapes(states, actions, gso)
        Ws, bs, gammas, betas = self.params()
        q = ops.critic(states, actions, gso, Ws, bs, gammas, betas, fused=self.use_fused)
        return q.view((batch_size, 1, n_agents))
