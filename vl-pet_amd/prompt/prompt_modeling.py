"""``InputPrompts`` (reference: prompt/prompt_modeling.py): ``prompt_len`` learned rows re-parametrised through a two-layer MLP,
``Embedding(P, d) -> Linear(d, mid) -> Tanh -> Linear(mid, d)``; state-dict keys ``prefix_embedding.{0,1,3}.{weight,bias}``.

The reference looks the P ids up once per batch item and runs the MLP on all B * P rows, although the result is the same for every
item.  ``rows()`` runs it on the P rows; ``get_prompt`` keeps the reference's signature and returns them as a stride-0 view."""
import torch
import torch.nn as nn


class InputPrompts(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.prompt_len = config.prompt_len
        self.input_dim = config.input_dim
        self.mid_dim = config.mid_dim
        self.prefix_tokens = torch.arange(self.prompt_len).long()      # (a plain attribute in the reference too: not in the state dict)
        self.prefix_embedding = nn.Sequential(
            nn.Embedding(self.prompt_len, self.input_dim),
            nn.Linear(self.input_dim, self.mid_dim),
            nn.Tanh(),
            nn.Linear(self.mid_dim, self.input_dim),
        )

    def rows(self) -> torch.Tensor:
        """[P, d]: the prompt of ONE batch item (the ids are 0 .. P - 1 in order, so the lookup is the embedding table itself)."""
        emb, down, act, up = self.prefix_embedding
        return up(act(down(emb.weight)))

    def get_prompt(self, bsz, device):
        rows = self.rows()
        if rows.device != torch.device(device):
            rows = rows.to(device)
        return rows.unsqueeze(0).expand(bsz, -1, -1)
