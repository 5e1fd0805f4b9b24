"""Adapter configuration: the attribute names ``AdapterController`` / ``Adapter`` read
(reference: adapters/config.py:4-55 and the assignments in trainer_base.py:141-178)."""
from dataclasses import dataclass, field
from typing import List, Optional


@dataclass
class AdapterConfig:
    # bottleneck
    non_linearity: str = "gelu_new"
    reduction_factor: int = 16
    use_adapter_down_dim: bool = False
    adapter_down_dim: int = 96
    input_dim: int = 768
    d_model: int = 768
    # controller
    tasks: Optional[List[str]] = None
    use_single_adapter: bool = False
    share_up_sampler: bool = False
    share_down_sampler: bool = False
    add_layer_norm_before_adapter: bool = False
    add_layer_norm_after_adapter: bool = False
    use_parallel_adapter: bool = False
    use_scaling_factor: bool = False
    scaling_factor: float = 1.0
    track_z: bool = False
    # a variant outside the hot path: low-rank adapters run as plain torch ops (eager fallback)
    low_rank_adapters: bool = False
    low_rank_w_init: str = "glorot-uniform"
    low_rank_rank: int = 1
    # Compacter (hypercomplex / PHM adapters, adapter_modeling.HyperComplexAdapter); defaults of the reference's CompactorConfig
    # (adapters/config.py:97-109), except ``hypercomplex_adapters`` / ``shared_phm_rule``, which the hosts set from their flags
    hypercomplex_adapters: bool = False
    hypercomplex_division: int = 4
    learn_phm: bool = True
    hypercomplex_nonlinearity: str = "glorot-uniform"
    shared_phm_rule: bool = False
    shared_phm_rule_over_tasks: bool = False
    factorized_phm: bool = True
    phm_c_init: str = "normal"
    phm_rank: int = 1
    phm_init_range: float = 0.0001
    # PHM forms no flag of the reference reaches: refused by HyperComplexAdapter with a ValueError that names the field
    shared_W_phm: bool = False
    factorized_phm_rule: bool = False
    kronecker_prod: bool = False


@dataclass
class MetaAdapterConfig(AdapterConfig):
    """Hyperformer: a hyper-network generates the adapters' weights from task and layer embeddings (reference: adapters/config.py:58-75,
    the class defaults; ``projected_task_embedding_dim`` is what ``--projected_task_embedding_dim`` sets, 8 in hyperformer.sh)."""
    task_embedding_dim: int = 512
    task_hidden_dim: int = 128
    projected_task_embedding_dim: int = 64
    unique_hyper_net: bool = True
    unique_hyper_net_layer_norm: bool = True
    efficient_unique_hyper_net: bool = False
    # forms no flag of the reference reaches: refused with a ValueError that names the field
    train_task_embeddings: bool = False
    task_to_embeddings: Optional[dict] = None
