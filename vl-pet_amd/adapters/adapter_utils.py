import torch
import torch.nn as nn

from ..activations import get_activation


class Activations(nn.Module):
    """Named activation (reference: adapters/adapter_utils.py:7-13)."""

    def __init__(self, activation_type: str):
        super().__init__()
        self.name = activation_type
        self.f = get_activation(activation_type)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.f(x)


def init_linear_layer(linear: nn.Linear, std: float = 1e-2) -> None:
    """N(0, std) weight, zero bias (reference: adapters/adapter_utils.py:16-19)"""
    nn.init.normal_(linear.weight, std=std)
    nn.init.zeros_(linear.bias)


def linear_layer(input_dim: int, output_dim: int, std: float = 1e-2) -> nn.Linear:
    linear = nn.Linear(input_dim, output_dim)
    init_linear_layer(linear, std=std)
    return linear


class TaskHyperNet(nn.Module):
    """The two-layer MLP that projects (task | layer id (| block type)) embeddings to ``projected_task_embedding_dim`` (reference:
    adapters/adapter_utils.py:29-43; the attribute keeps the reference's spelling, it is a state-dict key).  The reference flattens its
    input to one vector; here the last dimension is the concatenation and leading dimensions are rows (all layers at once)."""

    def __init__(self, config, input_dim: int):
        super().__init__()
        self.task_hidden_dim = config.task_hidden_dim
        self.projected_task_embedding_dim = config.projected_task_embedding_dim
        self.task_embeding_generator = nn.Sequential(linear_layer(input_dim, self.task_hidden_dim), nn.ReLU(),
                                                     linear_layer(self.task_hidden_dim, self.projected_task_embedding_dim))

    def forward(self, task_embedding: torch.Tensor) -> torch.Tensor:
        return self.task_embeding_generator(task_embedding)


class TaskEmbeddingController(nn.Module):
    """One ``randn`` embedding per task (reference: adapters/adapter_utils.py:60-91).  ``train_task_embeddings`` and
    ``task_to_embeddings`` are set by no launch script of the reference and are refused by name."""

    def __init__(self, config):
        super().__init__()
        if getattr(config, "train_task_embeddings", False):
            raise ValueError("train_task_embeddings is not supported (no launch flag of the reference reaches it)")
        if getattr(config, "task_to_embeddings", None) is not None:
            raise ValueError("task_to_embeddings is not supported (no launch flag of the reference reaches it)")
        self.task_embedding_dim = config.task_embedding_dim
        self.tasks = list(config.tasks)
        self.task_to_embeddings = nn.ParameterDict(dict())
        for task in self.tasks:         # (one at a time: the reference's order of keys and of draws from the generator)
            self.task_to_embeddings[task] = nn.Parameter(torch.randn(self.task_embedding_dim))

    def forward(self, task: str) -> torch.Tensor:
        return self.task_to_embeddings[task]
