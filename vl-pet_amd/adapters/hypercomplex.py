"""Compacter's PHM layer (reference: adapters/hypercomplex/layers.py:36-177; parameter names, shapes and init rules kept).

    PHMLinear(in, out, n):  phm_rule [n, n, n],  W [n, in / n, out / n] (or W_left [n, in / n, rank] and W_right [n, rank, out / n]),  b [out]
    H[a k + kk, c p + pp] = sum_i phm_rule[i, a, c] W[i, kk, pp]            y = x @ H + b

The module owns the parameters; ``forward`` is the plain-torch composition (vl-pet_amd/eager.py).  Inside an adapter the two layers'
weights are generated together by ``functional.phm_expand_pair`` (csrc/phm.hip) -- see adapter_modeling.HyperComplexAdapter."""
import math

import torch
import torch.nn as nn

W_INITS = ("glorot-normal", "glorot-uniform", "normal")
C_INITS = ("normal", "uniform")
UNREACHABLE = ("shared_W_phm", "factorized_phm_rule", "kronecker_prod")      # no flag of the reference sets them (param.py:148-170)


class PHMLinear(nn.Module):
    def __init__(self, in_features: int, out_features: int, phm_dim: int, bias: bool = True, w_init: str = "glorot-uniform",
                 c_init: str = "normal", learn_phm: bool = True, shared_phm_rule: bool = False, factorized_phm: bool = False,
                 shared_W_phm: bool = False, factorized_phm_rule: bool = False, phm_rank: int = 1, phm_init_range: float = 0.0001,
                 kronecker_prod: bool = False):
        super().__init__()
        for name, on in zip(UNREACHABLE, (shared_W_phm, factorized_phm_rule, kronecker_prod)):
            if on:
                raise ValueError(f"{name} is not supported (no launch flag of the reference reaches it)")
        if w_init not in W_INITS:
            raise ValueError(f"hypercomplex_nonlinearity {w_init!r}: one of {W_INITS}")
        if c_init not in C_INITS:
            raise ValueError(f"phm_c_init {c_init!r}: one of {C_INITS}")
        if phm_dim < 1 or in_features % phm_dim or out_features % phm_dim:
            raise ValueError(f"hypercomplex_division {phm_dim} does not divide {in_features} x {out_features}")
        self.in_features, self.out_features, self.phm_dim = in_features, out_features, phm_dim
        self.learn_phm, self.shared_phm_rule, self.factorized_phm = learn_phm, shared_phm_rule, factorized_phm
        self.phm_rank, self.phm_init_range, self.w_init, self.c_init = phm_rank, phm_init_range, w_init, c_init
        k, p = in_features // phm_dim, out_features // phm_dim
        if not shared_phm_rule:         # a shared rule is the model's: set_phm_rule() hands it in (and registers it under this name too)
            self.phm_rule = nn.Parameter(torch.empty(phm_dim, phm_dim, phm_dim), requires_grad=learn_phm)
        if factorized_phm:
            self.W_left = nn.Parameter(torch.empty(phm_dim, k, phm_rank))
            self.W_right = nn.Parameter(torch.empty(phm_dim, phm_rank, p))
        else:
            self.W = nn.Parameter(torch.empty(phm_dim, k, p))
        if bias:
            self.b = nn.Parameter(torch.empty(out_features))
        else:
            self.register_parameter("b", None)
        self.reset_parameters()

    def reset_parameters(self):
        """layers.py:98-149: every slice of W by its own Glorot rule with gain sqrt(2) (or N(0, phm_init_range)); zero bias; the rule
        N(0, phm_init_range) or U(-0.01, 0.01)"""
        with torch.no_grad():
            for w in ((self.W_left, self.W_right) if self.factorized_phm else (self.W,)):
                for i in range(self.phm_dim):
                    if self.w_init == "glorot-normal":
                        nn.init.xavier_normal_(w[i], gain=math.sqrt(2))
                    elif self.w_init == "glorot-uniform":
                        nn.init.xavier_uniform_(w[i], gain=math.sqrt(2))
                    else:
                        w[i].normal_(mean=0, std=self.phm_init_range)
            if self.b is not None:
                self.b.zero_()
            if not self.shared_phm_rule:
                if self.c_init == "uniform":
                    self.phm_rule.uniform_(-0.01, 0.01)
                else:
                    self.phm_rule.normal_(mean=0, std=self.phm_init_range)

    def set_phm_rule(self, phm_rule=None):
        self.phm_rule = phm_rule

    def slices(self) -> torch.Tensor:
        """W [n, k, p]; for factorized layers the product of the factors (a plain torch op in front of the expansion)"""
        if self.factorized_phm:
            from .. import eager
            return eager.phm_factors(self.W_left, self.W_right)
        return self.W

    def sources(self):
        """the parameters the expanded weight is made from (cache keys)"""
        return [self.phm_rule] + ([self.W_left, self.W_right] if self.factorized_phm else [self.W])

    def forward(self, x):
        from .. import eager
        return eager.phm_linear(x, self.phm_rule, self.slices(), self.b)
