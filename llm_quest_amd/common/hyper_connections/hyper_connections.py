"""Classic hyper-connections -- API of ``llm_quest/common/hyper_connections/hyper_connections.py``.

The three classes hold the coefficients of one connection under the reference's names, shapes, dtypes and initial values, so a
``state_dict`` moves between the two implementations.  They do NOT carry the arithmetic: a sub-block's norm, residual mixing,
pre-mapping and post-mapping run as two fused HIP kernels on either side of the sub-layer (``hyper_qwen3.py``,
``csrc/hyper_conn.hip``), which needs all three connections at once.
"""

import torch
import torch.nn as nn


class _HyperConnection(nn.Module):
    """``factor`` [1] (alpha, 0.01), ``linear.weight`` [rows, emb_dim] (dynamic mapping, zero), ``bias`` (static mapping) -- all kept in
    ``h_dtypes`` (fp32) through ``model.to(torch.bfloat16)``, as the reference's ``HCCoeffsFP32Mixin`` keeps them."""

    def __init__(self, emb_dim, rows, bias_init, add_static_mapping, activation_cls, device, h_dtypes):
        super().__init__()
        if activation_cls is not nn.Tanh:
            raise NotImplementedError(f"hyper-connections: activation {activation_cls!r} is not implemented (the fused kernels compute nn.Tanh only)")
        if h_dtypes != torch.float32:
            raise NotImplementedError(f"hyper-connections: h_dtypes {h_dtypes} is not implemented (the fused kernels keep every coefficient in fp32)")
        self.h_dtypes = h_dtypes
        self.activation = activation_cls()
        self.factor = nn.Parameter(torch.tensor([0.01], device=device, dtype=h_dtypes))
        self.linear = nn.Linear(emb_dim, rows, bias=False, device=device, dtype=h_dtypes)
        nn.init.zeros_(self.linear.weight)
        self.bias = nn.Parameter(bias_init.to(device=device, dtype=h_dtypes)) if add_static_mapping else None

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse=recurse)
        dt = self.h_dtypes
        self.factor.data = self.factor.data.to(dtype=dt)
        self.linear.weight.data = self.linear.weight.data.to(dtype=dt)
        if self.bias is not None:
            self.bias.data = self.bias.data.to(dtype=dt)
        return self

    def forward(self, x, x_norm):
        raise NotImplementedError(
            f"{type(self).__name__} holds coefficients only: the connections of a sub-block run fused inside HyperQwen3TransformerBlock; "
            "a stand-alone forward of one connection is not implemented"
        )


class HyperConnectionRes(_HyperConnection):
    """H_res @ x, the mixing of the n residual streams (bias: identity [n, n])."""

    def __init__(self, emb_dim, expansion_rate=4, add_static_mapping=True, activation_cls=nn.Tanh, device=None, h_dtypes=torch.float32):
        super().__init__(emb_dim, expansion_rate, torch.eye(expansion_rate), add_static_mapping, activation_cls, device, h_dtypes)


class HyperConnectionPre(_HyperConnection):
    """H_pre @ x, the n streams folded into the sub-layer's single input (bias: 1/n each)."""

    def __init__(self, emb_dim, expansion_rate=4, add_static_mapping=True, activation_cls=nn.Tanh, device=None, h_dtypes=torch.float32):
        super().__init__(emb_dim, 1, torch.ones(expansion_rate) / expansion_rate, add_static_mapping, activation_cls, device, h_dtypes)


class HyperConnectionPost(_HyperConnection):
    """H_post^T @ y, the sub-layer's output spread back over the n streams (bias: ones)."""

    def __init__(self, emb_dim, expansion_rate=4, add_static_mapping=True, activation_cls=nn.Tanh, device=None, h_dtypes=torch.float32):
        super().__init__(emb_dim, 1, torch.ones(expansion_rate), add_static_mapping, activation_cls, device, h_dtypes)
