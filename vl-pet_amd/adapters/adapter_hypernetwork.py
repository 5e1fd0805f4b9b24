"""Hyperformer's hyper-networks (reference: adapters/adapter_hypernetwork.py:35-261, adapters/adapter_controller.py:212-250; class
names, parameter names, state-dict keys and init rules kept): a stack's controller generates the weights of every adapter of every
layer from a task embedding and the layers' (and block types') embeddings.

The reference calls its controller once per layer, and that call runs an embedding lookup, a cat, the MLP, a LayerNorm and four
nn.Linear generators per block.  Here ``generate()`` produces ALL layers at once: the embedding chain runs once on the E rows in plain
torch (autograd owns its backward), then ONE ``functional.hyper_generate`` launch (csrc/hyper.hip) applies every generator to every
row.  Row l of a weight generator, viewed [r, d] / [d, r], is the nn.Linear layout K2 / K1 / adapter_tail take; the adapter itself is
the Single-Adapter placement with the weights handed in (``MetaLayersAdapterController.fused``).

Staleness rule of the generated weights and their packs (the one of ``adapter_modeling.HyperComplexAdapter``):
  * autograd on: generation and packs run in EVERY ``generate()`` (the packs into buffers this controller keeps).  A captured train
    step then contains them and reads the parameters in place.
    The packs are ONE buffer per (layer, block), shared by all tasks and all forwards: a second ``generate()`` before the first one's
    backward (gradient accumulation over two forwards) overwrites the packs the first backward reads -- run forward and backward in
    turn, as the trainer does (the same rule as ``HyperComplexAdapter``).
  * under ``no_grad`` with a ``task`` name: weights and packs are cached per (task, IO dtype) on (data_ptr, _version) of every source
    parameter and of the task embedding, ``functional.WEIGHTS_EPOCH`` and the dtype, and on a miss are refreshed INTO THE SAME
    BUFFERS, which belong to that task alone: a captured decode step of one task keeps reading valid, current memory and never another
    task's weights.  The hosts fetch a stack's weights ONCE per ``generate()`` call, before the decode loop and outside the captured
    step: that call is where a changed parameter is noticed; a replayed step only reads the buffers.  Without a ``task`` nothing is
    cached.
CPU tensors, a non-linearity other than gelu_new, ``track_z`` and geometries beyond the kernel's limits (functional.hyper_applies) run
the plain-torch composition (eager.hyper_generate, eager.adapter)."""
import torch
import torch.nn as nn

from .adapter_utils import Activations, TaskHyperNet, linear_layer
from .. import functional as VF

BLOCKS = ("self_attention", "feed_forward", "cross_attention")
BLOCK_TYPE_ID = {"feed_forward": 0, "self_attention": 1, "cross_attention": 2}        # adapter_hypernetwork.py:215-230
REFUSED = ("add_layer_norm_before_adapter", "add_layer_norm_after_adapter")            # the LayerNormHyperNet path


class AdapterWeights:
    """One adapter's generated set: down weight [r, d], down bias [r], up weight [d, r], up bias [d] and, on the kernel path, their
    pack for one IO dtype."""

    __slots__ = ("down_w", "down_b", "up_w", "up_b", "pack")

    def __init__(self, down_w, down_b, up_w, up_b, pack=None):
        self.down_w, self.down_b, self.up_w, self.up_b, self.pack = down_w, down_b, up_w, up_b, pack

    def tail_weights(self):
        """(down weight, down bias, up weight, up bias) as ``adapter_tail.adapter_tail`` reads them"""
        return self.down_w, self.down_b, self.up_w, self.up_b


class AdapterLayersHyperNet(nn.Module):
    """Weight and bias generator of one projection: nn.Linear(P -> input_dim * output_dim) and nn.Linear(P -> input_dim), the generated
    weight being [input_dim, output_dim] = nn.Linear's [out, in] (adapter_hypernetwork.py:35-51)."""

    def __init__(self, config, input_dim: int, output_dim: int):
        super().__init__()
        self.input_dim, self.output_dim = input_dim, output_dim
        self.weight_generator = nn.Sequential(linear_layer(config.projected_task_embedding_dim, input_dim * output_dim))
        self.bias_generator = nn.Sequential(linear_layer(config.projected_task_embedding_dim, input_dim))

    def maps(self):
        return [(self.weight_generator[0].weight, self.weight_generator[0].bias), (self.bias_generator[0].weight, self.bias_generator[0].bias)]

    def forward(self, embeddings):
        return self.weight_generator(embeddings).view(self.input_dim, self.output_dim), self.bias_generator(embeddings).view(-1)


class _HyperNetController(nn.Module):
    """What both controller forms share: the refused flags, the layer-id embeddings, the MLP and its LayerNorm, the batched
    ``generate()`` with its caches.  A subclass says which rows exist (``embedding_inputs``), which maps (``hyper_nets``) and where one
    adapter's four results sit (``locate``)."""

    def __init__(self, config, num_layers: int, include_cross_attention: bool, n_embeddings: int):
        super().__init__()
        for name in REFUSED:
            if getattr(config, name, False):
                raise ValueError(f"{name} with use_hyperformer (the LayerNormHyperNet path) is not supported: no launch script of the "
                                 f"reference sets it")
        if getattr(config, "train_task_embeddings", False):
            raise ValueError("train_task_embeddings is not supported (no launch flag of the reference reaches it)")
        self.num_layers = num_layers
        self.layer_norm_epsilon = 1e-6
        self.task_embedding_dim = config.task_embedding_dim
        self.include_cross_attention = include_cross_attention
        self.blocks = BLOCKS if include_cross_attention else BLOCKS[:2]
        self.layer_id_embeddings = nn.Embedding(num_layers, self.task_embedding_dim)
        self._n_embeddings = n_embeddings

    def _finish_init(self, config):
        """(the reference's registration order: embeddings, MLP, LayerNorm, then the generators)"""
        self.task_hypernet = TaskHyperNet(config, input_dim=self.task_embedding_dim * self._n_embeddings)
        self.unique_hyper_net_layer_norm = bool(config.unique_hyper_net_layer_norm)
        if self.unique_hyper_net_layer_norm:
            self.LayerNorm = nn.LayerNorm(config.projected_task_embedding_dim, eps=self.layer_norm_epsilon)
        self.input_dim = config.input_dim
        self.down_sample_size = self.input_dim // config.reduction_factor
        self.projected_dim = config.projected_task_embedding_dim
        self.eager = config.non_linearity.lower() != "gelu_new" or bool(getattr(config, "track_z", False))
        self._train_packs = {}      # autograd on: (layer, block) -> the one buffer every generate() packs into
        self._cache = {}            # no_grad: (task, io_dtype) -> [key, outs, {(layer, block): pack}]

    # -- the embedding chain: plain torch on the E rows
    def embedding_inputs(self, task_embedding):
        raise NotImplementedError

    def project(self, rows):
        e = self.task_hypernet(rows)
        return self.LayerNorm(e) if self.unique_hyper_net_layer_norm else e

    def embedding_rows(self, task_embedding):
        """[E, P]: the projected embedding of every (layer (, block type)) under this task"""
        return self.project(self.embedding_inputs(task_embedding))

    def hyper_nets(self):
        raise NotImplementedError

    def locate(self, layer, block):
        """-> (row of the embeddings, index of the adapter's first map: down weight, down bias, up weight, up bias follow each other)"""
        raise NotImplementedError

    def maps(self):
        return [m for net in self.hyper_nets() for m in net.maps()]

    def _sources(self, task_embedding):
        return [task_embedding] + list(self.parameters())

    def _kernel_path(self, task_embedding) -> bool:
        maps = self.maps()
        return (not self.eager and task_embedding.is_cuda and maps[0][0].is_cuda
                and VF.hyper_applies(len(maps), self.n_rows, self.projected_dim, maps[0][0].dtype))

    def _collect(self, rows, packs):
        r, d = self.down_sample_size, self.input_dim
        out = []
        for layer in range(self.num_layers):
            per = {}
            for block in self.blocks:
                row, base = self.locate(layer, block)
                per[block] = AdapterWeights(rows[base][row].view(r, d), rows[base + 1][row], rows[base + 2][row].view(d, r),
                                            rows[base + 3][row], None if packs is None else packs.get((layer, block)))
            out.append(per)
        return out

    def _pack_all(self, weights, store, io_dtype):
        for layer, per in enumerate(weights):
            for block, w in per.items():
                store[(layer, block)] = w.pack = VF.pack_pair([w.down_w], [w.down_b], w.up_w, w.up_b, io_dtype, out=store.get((layer, block)))

    def generate(self, task_embedding, task=None, io_dtype=None):
        """Every layer's adapters under ``task_embedding``: a list over layers of {block: AdapterWeights}.  ``io_dtype``
        (functional._io_dtype of the activations): pack each adapter for K2 / K1 as well.  ``task``: the name the no_grad cache files
        this result under; without it nothing is cached."""
        if not self._kernel_path(task_embedding):
            from .. import eager
            return self._collect(eager.hyper_generate(self.maps(), self.embedding_rows(task_embedding)), None)
        if torch.is_grad_enabled():
            rows = VF.hyper_generate(self.maps(), self.embedding_rows(task_embedding).float())
            weights = self._collect(rows, None)
            if io_dtype is not None:
                self._pack_all(weights, self._train_packs, io_dtype)
            return weights
        if task is None:            # nothing to file the result under: not cached (fresh buffers, nothing a captured graph could hold)
            outs = VF.hyper_generate_into(self.maps(), self.embedding_rows(task_embedding).float())
            weights = self._collect(outs, None)
            if io_dtype is not None:
                self._pack_all(weights, {}, io_dtype)
            return weights
        srcs = self._sources(task_embedding)
        key = (VF.WEIGHTS_EPOCH, srcs[1].dtype) + tuple((t.data_ptr(), t._version) for t in srcs)
        slot = self._cache.setdefault((task, io_dtype), [None, None, {}])
        if slot[0] != key:
            slot[1] = VF.hyper_generate_into(self.maps(), self.embedding_rows(task_embedding).float(), out=slot[1])
            weights = self._collect(slot[1], None)
            if io_dtype is not None:
                self._pack_all(weights, slot[2], io_dtype)
            slot[0] = key
        return self._collect(slot[1], slot[2] if io_dtype is not None else None)

    def forward(self, task_embedding, layer_id):
        """One layer's adapters as the reference computes them, call by call in plain torch: {block: AdapterWeights} (the reference's
        AdapterT5BlockOutput).  The hosts use ``generate()``."""
        out = {}
        for block in self.blocks:
            e = self.get_embedding(task_embedding, layer_id, block)
            down, up = self.block_nets(block)
            (dw, db), (uw, ub) = down(e), up(e)
            out[block] = AdapterWeights(dw, db, uw, ub)
        return out


class AdapterLayersHyperNetController(_HyperNetController):
    """``--unique_hyper_net``: one pair of generators per block type, one embedding row per layer (adapter_hypernetwork.py:54-155).
    S = 8 maps (12 with cross-attention), E = num_layers."""

    def __init__(self, config, num_layers: int = 6, include_cross_attention: bool = False):
        super().__init__(config, num_layers, include_cross_attention, n_embeddings=2)
        self._finish_init(config)
        d, r = self.input_dim, self.down_sample_size
        self.feed_forward_up_sampler_hyper_net = AdapterLayersHyperNet(config, d, r)
        self.feed_forward_down_sampler_hyper_net = AdapterLayersHyperNet(config, r, d)
        self.self_attention_up_sampler_hyper_net = AdapterLayersHyperNet(config, d, r)
        self.self_attention_down_sampler_hyper_net = AdapterLayersHyperNet(config, r, d)
        if include_cross_attention:
            self.cross_attention_up_sampler_hyper_net = AdapterLayersHyperNet(config, d, r)
            self.cross_attention_down_sampler_hyper_net = AdapterLayersHyperNet(config, r, d)
        self.n_rows = num_layers

    def block_nets(self, block):
        return getattr(self, block + "_down_sampler_hyper_net"), getattr(self, block + "_up_sampler_hyper_net")

    def hyper_nets(self):
        return [net for block in self.blocks for net in self.block_nets(block)]

    def locate(self, layer, block):
        return layer, 4 * self.blocks.index(block)

    def embedding_inputs(self, task_embedding):
        t = task_embedding.view(1, -1).expand(self.num_layers, -1)
        return torch.cat([t, self.layer_id_embeddings.weight], dim=1)

    def get_embedding(self, task_embedding, layer_id, block=None):
        """adapter_hypernetwork.py:107-117"""
        return self.project(torch.cat([task_embedding.view(-1), self.layer_id_embeddings.weight[layer_id]]))


class AdapterLayersOneHyperNetController(_HyperNetController):
    """``--efficient_unique_hyper_net``: ONE pair of generators for every block type, one embedding row per layer and block type
    (adapter_hypernetwork.py:158-261).  S = 4 maps, E = num_layers x 2 (3 with cross-attention), rows layer-major."""

    def __init__(self, config, num_layers: int = 6, include_cross_attention: bool = False):
        super().__init__(config, num_layers, include_cross_attention, n_embeddings=3)
        self.adapters_block_type = nn.Embedding(3, self.task_embedding_dim)
        self._finish_init(config)
        self.up_sampler_hyper_net = AdapterLayersHyperNet(config, self.input_dim, self.down_sample_size)
        self.down_sampler_hyper_net = AdapterLayersHyperNet(config, self.down_sample_size, self.input_dim)
        self.n_rows = num_layers * len(self.blocks)

    def block_nets(self, block):
        return self.down_sampler_hyper_net, self.up_sampler_hyper_net

    def hyper_nets(self):
        return [self.down_sampler_hyper_net, self.up_sampler_hyper_net]

    def locate(self, layer, block):
        return layer * len(self.blocks) + self.blocks.index(block), 0

    def embedding_inputs(self, task_embedding):
        # (views, a stack and a cat only: an index tensor made from a Python list would be a host-to-device copy, which a stream
        # capture refuses)
        L, nb, T = self.num_layers, len(self.blocks), self.task_embedding_dim
        types = torch.stack([self.adapters_block_type.weight[BLOCK_TYPE_ID[b]] for b in self.blocks])
        return torch.cat([task_embedding.view(1, 1, T).expand(L, nb, T), self.layer_id_embeddings.weight.view(L, 1, T).expand(L, nb, T),
                          types.view(1, nb, T).expand(L, nb, T)], dim=2).view(L * nb, 3 * T)

    def get_embedding(self, task_embedding, layer_id, block):
        """adapter_hypernetwork.py:198-212"""
        return self.project(torch.cat([task_embedding.view(-1), self.layer_id_embeddings.weight[layer_id],
                                       self.adapters_block_type.weight[BLOCK_TYPE_ID[block]]]))


class MetaLayersAdapterController(nn.Module):
    """Applies an adapter whose weights are handed in (adapter_controller.py:212-250); it has no parameters.  ``forward`` is the
    reference's: adapter(inputs) + inputs.  ``fused`` is the Single-Adapter placement's call: residual + scale * adapter(x) in one K2
    launch when the weights came with a pack."""

    def __init__(self, config):
        super().__init__()
        for name in REFUSED:
            if getattr(config, name, False):
                raise ValueError(f"{name} with use_hyperformer (the LayerNormHyperNet path) is not supported: no launch script of the "
                                 f"reference sets it")
        self.activation_type = config.non_linearity.lower()
        self.activation = Activations(self.activation_type)
        self.input_dim = config.input_dim
        self.track_z = bool(getattr(config, "track_z", False))
        self.eager = self.activation_type != "gelu_new" or self.track_z

    def _keep_z(self, z):
        if self.track_z:
            self.z = z

    def call_adapter(self, inputs, w: AdapterWeights):
        from .. import eager
        return eager.adapter(inputs, w.down_w, w.down_b, w.up_w, w.up_b, self.activation, self._keep_z)

    def fused(self, x, residual, w: AdapterWeights, scale=1.0, link=None):
        if self.eager or not x.is_cuda or w.pack is None:
            out = self.call_adapter(x, w)
            return residual + (out if scale == 1.0 else scale * out)
        return VF.parallel_adapter(x, residual, w.down_w, w.down_b, w.up_w, w.up_b, w.pack, scale, link=link)

    def forward(self, inputs, adapter_weights: AdapterWeights):
        return self.fused(inputs, inputs, adapter_weights)
