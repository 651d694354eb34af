"""Learned-query cross-attention: the IPS patch scorer and the patch aggregator.

Drop-in mirror of /root/reference/architecture/transformer.py - same public
names (``pos_enc_1d``, ``ScaledDotProductAttention``, ``MultiHeadCrossAttention``,
``MLP``, ``Transformer``), constructor arguments, parameter names and shapes, so
state-dicts interchange with the reference.

Three execution paths live behind that interface:

* tensors on a ROCm device, autograd off  ->  the hand-written gfx950 kernels in
  ``ips_amd/csrc`` through the C ABI of ``include/ipsx.h`` (``ips_amd.hip``).
  There is no fallback: if ``libipsx.so`` is missing the call raises.
* tensors on a ROCm device, autograd on, ``Transformer.forward``  ->  the attention pool on folded queries as one
  autograd node (``ips_amd/training/fused_aggregator.py``, csrc/attn_pool_train.hip), the R-row rest on stock ops.
* everything else (CPU tensors, ``get_scores`` / ``get_attn`` under autograd, ``IPSX_TRAIN_AGGREGATOR=0``)
  ->  stock ATen ops, which is what the reference itself dispatches.

``Transformer.forward(x, count=)`` (not in the reference) masks the zero padding of a ``pad=True`` batch on
each of the three paths; ``count=None`` is the code above, unchanged.
"""

import math

import torch
from torch import nn

from .. import hip


def pos_enc_1d(D, len_seq):
    """Sinusoidal table ``(len_seq, D)``; reference transformer.py:6-18.

    Built with the same ATen ops in the same order as the reference so the
    table is bit-identical to it on CPU (it is data for the kernels, which
    gather rows of it by patch index).
    """
    if D % 2:
        raise ValueError("Cannot use sin/cos positional encoding with "
                         "odd dim (got dim={:d})".format(D))
    freq = torch.exp(torch.arange(0, D, 2, dtype=torch.float) * -(math.log(10000.0) / D))
    phase = torch.arange(0, len_seq).unsqueeze(1).float() * freq
    table = torch.zeros(len_seq, D)
    table[:, 0::2] = torch.sin(phase)
    table[:, 1::2] = torch.cos(phase)
    return table


def _use_hip(*tensors):
    """HIP kernels run when data is on the GPU and no autograd graph is wanted."""
    if not tensors[0].is_cuda:
        return False
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors if t is not None):
        return False
    return hip.backend() == "hip"


class ScaledDotProductAttention(nn.Module):
    """softmax(q/temperature . k^T) [. v]; reference transformer.py:20-41."""

    def __init__(self, temperature, attn_dropout=0.1):
        super().__init__()
        self.temperature = temperature
        self.dropout = nn.Dropout(attn_dropout)

    def compute_attn(self, q, k, count=None):
        """``count`` (not in the reference; an integer tensor (B,) on k's device, None = every slot): slide b attends to its
        slots 0 .. count[b] - 1 only - the others are filled with -inf in front of the softmax, so their probability is
        exactly +0.0 and their gradient exactly 0.  This is the definition the masked kernels are held to."""
        # the division is applied to q BEFORE the contraction (reference :31)
        logits = torch.matmul(q / self.temperature, k.transpose(2, 3))
        if count is not None:
            beyond = torch.arange(k.shape[2], device=k.device)[None, :] >= count.to(k.device)[:, None]          # (B, M)
            logits = logits.masked_fill(beyond[:, None, None, :], float("-inf"))
        return self.dropout(torch.softmax(logits, dim=-1))

    def forward(self, q, k, v, count=None):
        return torch.matmul(self.compute_attn(q, k, count), v)


class MultiHeadCrossAttention(nn.Module):
    """``n_token`` learned queries attend over the patch embeddings.

    Reference transformer.py:43-109.  Parameters: ``q`` (1, n_token, D) and
    bias-free ``q_w``, ``k_w`` (H*D_k, D), ``v_w`` (H*D_v, D), ``fc`` (D, H*D_v),
    ``layer_norm`` (eps 1e-6).
    """

    def __init__(self, n_token, H, D, D_k, D_v, attn_dropout=0.1, dropout=0.1):
        super().__init__()
        self.n_token, self.H, self.D_k, self.D_v = n_token, H, D_k, D_v

        self.q = nn.Parameter(torch.empty((1, n_token, D)))
        bound = math.sqrt(1 / D_k)
        nn.init.uniform_(self.q, a=-bound, b=bound)

        self.q_w = nn.Linear(D, H * D_k, bias=False)
        self.k_w = nn.Linear(D, H * D_k, bias=False)
        self.v_w = nn.Linear(D, H * D_v, bias=False)
        self.fc = nn.Linear(H * D_v, D, bias=False)

        self.attention = ScaledDotProductAttention(temperature=D_k ** 0.5, attn_dropout=attn_dropout)
        self.dropout = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(D, eps=1e-6)

    def _heads(self, proj, x, width):
        b, length = x.shape[:2]
        return proj(x).view(b, length, self.H, width).transpose(1, 2)

    def scaled_query(self):
        """(n_token, H*D_k) query projection already divided by the temperature.

        Constant for a whole ``ips()`` call; the HIP scan keeps it in LDS.
        """
        return hip.query_proj(self.q[0], self.q_w.weight, self.attention.temperature)

    def folded_query(self):
        """The scaled query folded into the key weights: packed (H*n_token, D) operand of ``hip.logits``.

        Depends on the three parameters only, so it is kept until one of them changes (in-place updates bump
        ``_version``; ``.to()`` / ``load_state_dict`` change the storage) - an evaluation loop folds once."""
        half = hip.precision() == "bf16"          # BASELINE configs[4]: the logits on the bf16 matrix pipe as well
        key = (hip.weights_generation(), half) + tuple((t.data_ptr(), t._version, t.device)
                                                        for t in (self.q, self.q_w.weight, self.k_w.weight))
        cached = getattr(self, "_folded", None)
        if cached is None or cached[0] != key:
            fold = hip.fold_query_bf16 if half else hip.fold_query
            cached = (key, fold(self.scaled_query(), self.k_w.weight, self.H, self.D_k, self.n_token))
            self._folded = cached
        return cached[1]

    def packed_v(self):
        """``v_w.weight`` in the matrix cores' operand layout (``hip.pack_linear``), kept until the parameter changes."""
        w = self.v_w.weight
        key = (hip.weights_generation(), w.data_ptr(), w._version, w.device)
        cached = getattr(self, "_packed_v", None)
        if cached is None or cached[0] != key:
            cached = self._packed_v = (key, hip.pack_linear(w))
        return cached[1]

    def get_attn(self, x):
        """Attention map ``(B, H, n_token, L)`` of the queries over ``x`` (B, L, D)."""
        if _use_hip(x, self.q, self.q_w.weight, self.k_w.weight) and not self._drops():
            return hip.attn_map(x, self.scaled_query(), self.k_w.weight, self.H, self.D_k, self.n_token)
        q = self._heads(self.q_w, self.q, self.D_k)
        k = self._heads(self.k_w, x, self.D_k)
        return self.attention.compute_attn(q, k)

    def _drops(self):
        return self.training and (self.dropout.p > 0 or self.attention.dropout.p > 0)

    def forward(self, x, count=None):
        b = x.shape[0]
        q = self._heads(self.q_w, self.q, self.D_k)
        k = self._heads(self.k_w, x, self.D_k)
        v = self._heads(self.v_w, x, self.D_v)
        ctx = self.attention(q, k, v) if count is None else self.attention(q, k, v, count)          # (B, H, n_token, D_v)
        ctx = ctx.transpose(1, 2).contiguous().view(b, self.n_token, -1)
        out = self.dropout(self.fc(ctx))
        out += self.q                                        # residual on the learned queries
        return self.layer_norm(out)


class MLP(nn.Module):
    """D -> D_inner -> D feed-forward with residual + LayerNorm; reference :111-132."""

    def __init__(self, D, D_inner, dropout=0.1):
        super().__init__()
        self.w_1 = nn.Linear(D, D_inner)
        self.w_2 = nn.Linear(D_inner, D)
        self.layer_norm = nn.LayerNorm(D, eps=1e-6)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x):
        y = self.dropout(self.w_2(torch.relu(self.w_1(x))))
        y += x
        return self.layer_norm(y)


class Transformer(nn.Module):
    """Cross-attention block + MLP; reference transformer.py:134-152."""

    def __init__(self, n_token, H, D, D_k, D_v, D_inner, attn_dropout=0.1, dropout=0.1):
        super().__init__()
        self.crs_attn = MultiHeadCrossAttention(n_token, H, D, D_k, D_v,
                                                attn_dropout=attn_dropout, dropout=dropout)
        self.mlp = MLP(D, D_inner, dropout=dropout)

    def get_scores(self, x):
        """Per-patch score ``(B, L)``: attention averaged over heads, then over tokens."""
        ca = self.crs_attn
        if _use_hip(x, ca.q, ca.q_w.weight, ca.k_w.weight) and not ca._drops():
            return hip.scores(x, ca.scaled_query(), ca.k_w.weight, ca.H, ca.D_k, ca.n_token)
        attn = ca.get_attn(x)
        return attn.mean(dim=1).transpose(1, 2).mean(-1)

    def forward(self, x, count=None):
        """Aggregate ``x`` (B, M, D) into ``(B, n_token, D)``.

        ``count`` (not in the reference; B ints or an integer tensor (B,), ``IPSNet.last_mem_count`` after a ``pad=True``
        selection; None = today's code on every route): slide b is aggregated from its slots 0 .. count[b] - 1 only, as
        ``self(x[b:b + 1, :count[b]])`` would - on every route, chosen as without it.  Host counts outside 1 .. M or of
        another length than B raise ValueError; a tensor on the GPU is not read back (``hip.slot_counts``)."""
        masked = {}
        if count is not None:
            if x.dim() != 3:
                raise ValueError("count needs x (B, M, D), got {}".format(tuple(x.shape)))
            # (ONE int32 tensor on x's device, checked once; the calls below get it as a keyword the unmasked ones never see)
            masked["count"] = hip.slot_counts("Transformer.forward", count, x.shape[0], x.shape[1], x.device)
        if _use_hip(x, *self.parameters()) and not self.training:
            return hip.aggregate(self, x, **masked)
        if (x.is_cuda and x.dim() == 3 and x.dtype == torch.float32 and torch.is_grad_enabled() and hip.backend() == "hip"
                and (x.requires_grad or any(p.requires_grad for p in self.parameters()))):
            # training step (reference training/iterative.py:158-163): the (B, M) part as one node on folded queries
            from ..training import fused_aggregator
            if fused_aggregator.enabled():
                if getattr(self, "_fused_train_ok", None) is None:        # (the module tree does not change after construction)
                    self._fused_train_ok = fused_aggregator.supported(self)
                if self._fused_train_ok:
                    return fused_aggregator.forward(self, x, **masked)
        return self.mlp(self.crs_attn(x, **masked))
