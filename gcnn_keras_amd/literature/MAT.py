"""MAT model builder (mirror of kgcnn/literature/MAT.py:23-205, ``make_model``), ragged from the input cast to the output.

The reference pads everything to ``(batch, max_atoms, ...)`` and carries masks; padding rows influence nothing there
(``h`` is 0 on them and every update is masked), so the ragged form below is the same function: every attention sub-block
is ``FusedMATBlock`` (layers/conv/mat_conv.py) where the sizes fit (``model.fused_attention_blocks``) - layer
normalisation, one packed q|k|v ``Dense`` and one ``mp_mat_attention_f32`` with the merge and residual epilogue, three
engine calls - and the layer sequence otherwise and with ``model.use_fused_attention = False``: layer normalisation, per
head three ``Dense`` and one attention launch, the concatenation or sum, the merging ``Dense`` and the residual add.

The reference as it executes, including its quirks:

* the edge-embedding test and ``has_edge_dim`` read ``inputs[1]["shape"]`` (the coordinates), so edges are never embedded
  and a ``Dense(1, use_bias=False)`` always maps the adjacency features to one value; that ``Dense`` is linear and commutes
  with the scatter-add, so it runs on the ``(M, Fe)`` edge values and gives the per-edge weight.  A rank-1 edge input
  raises ``NotImplementedError`` (in the reference that ``Dense`` would act over the padded atom axis);
* ``max_atoms``: ``None`` or at least the largest molecule of the batch; smaller raises ``ValueError`` (the reference
  truncates molecules, which is not built);
* ``output_embedding="node"`` returns the padded ``(batch, max_atoms or Nmax, out)`` tensor with zero rows on padding;
  ``"graph"`` is the segment sum of ``MATGlobalPool`` (one row per graph, empty graphs included) and the output ``MLP``.

Weight order (``get_weights()``): node embedding, the width-fixing ``Dense``, the adjacency ``Dense(1)`` (it has the
graph depth of the first layer normalisation in Keras' ordering), then per depth LN, heads x (q, k, v kernel + bias),
merge ``Dense``, LN, ``MLP``, ``Dense``, then the final LN and the output ``MLP``.  Inference only (mat_conv.py).
"""
import numpy as np
import torch

from .. import _ffi
from ..layers.conv.mat_conv import (MERGE_SUM_NAMES, FusedMATBlock, MATAttentionHead, MATDistanceMatrix, MATGlobalPool,
                                    _refuse_grad)
from ..layers.mlp import MLP, GraphMLP
from ..layers.modules import Dense, LazyAdd, LazyConcatenate, OptionalInputEmbedding
from ..layers.norm import GraphLayerNormalization
from ..model.utils import RouteSwitchModel, update_model_kwargs

__model_version__ = "2022.11.25"

model_default = {
    "name": "MAT",
    "inputs": [
        {"shape": (None,), "name": "node_number", "dtype": "float32", "ragged": True},
        {"shape": (None, 3), "name": "node_coordinates", "dtype": "float32", "ragged": True},
        {"shape": (None, 1), "name": "edge_weights", "dtype": "float32", "ragged": True},
        {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}
    ],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64},
                        "edge": {"input_dim": 95, "output_dim": 64}},
    "use_edge_embedding": False,
    "max_atoms": None,
    "distance_matrix_kwargs": {"trafo": "exp"},
    "attention_kwargs": {"units": 8, "lambda_attention": 0.3, "lambda_distance": 0.3, "lambda_adjacency": None,
                         "dropout": 0.1, "add_identity": False},
    "feed_forward_kwargs": {"units": [32, 32, 32], "activation": ["relu", "relu", "linear"]},
    "embedding_units": 32,
    "depth": 5,
    "heads": 8,
    "merge_heads": "concat",
    "verbose": 10,
    "pooling_kwargs": {"pooling_method": "sum"},
    "output_embedding": "graph",
    "output_to_tensor": True,
    "output_mlp": {"use_bias": [True, True, True], "units": [32, 16, 1],
                   "activation": ["relu", "relu", "linear"]}
}


class _MatModel(RouteSwitchModel):
    """``Model`` with the ``use_fused_attention`` switch over all attention heads."""

    switch_attr, switch_layers_attr = "use_fused_attention", "attention_heads"
    attention_heads = ()
    use_fused_attention = RouteSwitchModel.switch


def _padded_nodes(out, max_atoms):
    """``(batch, max_atoms or Nmax, F)`` with zero rows on padding: ``mp_ragged_to_padded_f32`` plus a zero pad."""
    splits = out.row_splits_host()
    g = out.nrows()
    nmax = int((splits[1:] - splits[:-1]).max()) if g > 0 else 0
    vals = out.values.contiguous()
    width = int(vals.shape[1])
    padded = torch.empty((g, nmax, width), dtype=torch.float32, device=vals.device)
    _ffi.call("mp_ragged_to_padded_f32", _ffi.ptr(vals), _ffi.ptr(out.row_splits), g, nmax, max(width, 1),
              _ffi.ptr(padded), None, _ffi.stream())
    if max_atoms and max_atoms > nmax:
        padded = torch.nn.functional.pad(padded, (0, 0, 0, max_atoms - nmax))
    return padded


@update_model_kwargs(model_default)
def make_model(name: str = None, inputs: list = None, input_embedding: dict = None, use_edge_embedding: bool = None,
               distance_matrix_kwargs: dict = None, attention_kwargs: dict = None, feed_forward_kwargs: dict = None,
               embedding_units: int = None, depth: int = None, heads: int = None, merge_heads: str = None,
               max_atoms: int = None, verbose: int = None, pooling_kwargs: dict = None, output_embedding: str = None,
               output_to_tensor: bool = None, output_mlp: dict = None):
    r"""Build MAT (kgcnn/literature/MAT.py:113-205).  Model inputs ``[node_attributes, node_coordinates,
    edge_attributes, edge_indices]``, all ragged.  ``model.fused_attention_blocks`` lists which attention sub-blocks fit
    the fused kernel, ``model.use_fused_attention`` switches the route of all of them."""
    if output_embedding not in ("graph", "node"):
        raise ValueError("Unsupported graph embedding for mode `MAT`")
    if len(inputs[2]["shape"]) < 2:
        raise NotImplementedError("MAT: the edge input needs a feature axis, e.g. shape (None, 1); on a rank-1 edge "
                                  "input the reference's Dense(1) acts over the padded atom axis, which has no ragged "
                                  "meaning")
    embed_n = OptionalInputEmbedding(**input_embedding["node"], use_embedding=len(inputs[0]["shape"]) < 2)
    # the reference tests inputs[1] (the coordinates, rank 2) here: the edges are never embedded
    embed_e = OptionalInputEmbedding(**input_embedding["edge"],
                                     use_embedding=len(inputs[1]["shape"]) < 2 and use_edge_embedding)
    dist = MATDistanceMatrix(**distance_matrix_kwargs)   # never called: the heads take its trafo
    dense0 = Dense(units=embedding_units, use_bias=False)
    adj_dense = Dense(1, use_bias=False)
    sum_heads = merge_heads in MERGE_SUM_NAMES
    combine = LazyAdd() if sum_heads else LazyConcatenate(axis=-1)
    add = LazyAdd()
    blocks = []
    for _ in range(depth):
        blk = {"ln1": GraphLayerNormalization(epsilon=1e-3),
               "heads": [MATAttentionHead(**attention_kwargs) for _ in range(heads)],
               "merge": Dense(units=embedding_units, use_bias=False),
               "ln2": GraphLayerNormalization(epsilon=1e-3),
               "mlp": MLP(**feed_forward_kwargs),
               "dense": Dense(units=embedding_units, use_bias=False)}
        for head in blk["heads"]:
            head.trafo = dist.trafo
        blk["fused"] = FusedMATBlock(blk["heads"], blk["merge"], merge_heads)
        blocks.append(blk)
    ln_out = GraphLayerNormalization(epsilon=1e-3)
    pool = MATGlobalPool(**pooling_kwargs) if output_embedding == "graph" else None
    out_mlp = MLP(**output_mlp) if output_embedding == "graph" else GraphMLP(**output_mlp)

    def forward(model_inputs, **kwargs):
        node_input, xyz, edge_input, edi = model_inputs
        if torch.is_grad_enabled():   # neither route has a reverse pass: say so here, not in whichever layer meets it first
            _refuse_grad(node_input.values, xyz.values, edge_input.values, *[t for lay in layers for _, t in lay.weights])
        if max_atoms:
            lengths = np.diff(node_input.row_splits_host())   # host copy cached on the input: one read per batch
            largest = int(lengths.max()) if lengths.size else 0
            if largest > max_atoms:
                raise ValueError("MAT: max_atoms=%d is smaller than the largest molecule of the batch (%d atoms); "
                                 "truncating molecules is not built" % (max_atoms, largest))
        if edge_input.values.dim() != 2:
            raise NotImplementedError("MAT: the edge input needs a feature axis (batch, [M], F)")
        nd = embed_n(node_input)
        w = adj_dense(embed_e(edge_input))          # (batch, [M], 1): Dense(1) commutes with the scatter-add
        h = dense0(nd)
        for blk in blocks:
            hn = blk["ln1"](h)
            if blk["fused"].route(hn, h, kwargs):
                h = blk["fused"](hn, h, xyz, w, edi)
            else:
                hs = [head([hn, xyz, w, edi]) for head in blk["heads"]]
                hu = blk["merge"](combine(hs) if len(hs) > 1 else hs[0])
                h = add([h, hu])
            hu = blk["dense"](blk["mlp"](blk["ln2"](h)))
            h = add([h, hu])
        out = ln_out(h)
        if output_embedding == "graph":
            return out_mlp(pool(out))
        return _padded_nodes(out_mlp(out), max_atoms)

    node_width = input_embedding["node"]["output_dim"] if len(inputs[0]["shape"]) < 2 else inputs[0]["shape"][-1]
    embed_n.ensure_built((None, None))
    embed_e.ensure_built((None, None))
    dense0.ensure_built((None, None, node_width))
    adj_dense.ensure_built((None, None, inputs[2]["shape"][-1]))
    units = attention_kwargs["units"]
    for blk in blocks:
        blk["ln1"].ensure_built((None, None, embedding_units))
        for head in blk["heads"]:
            head.ensure_built([(None, None, embedding_units), (None, None, 3), (None, None, 1), (None, None, 2)])
        blk["merge"].ensure_built((None, None, units if sum_heads else units * heads))
        blk["ln2"].ensure_built((None, None, embedding_units))
        blk["mlp"].ensure_built((None, None, embedding_units))
        blk["dense"].ensure_built((None, None, feed_forward_kwargs["units"][-1]
                                   if isinstance(feed_forward_kwargs["units"], (list, tuple))
                                   else feed_forward_kwargs["units"]))
    ln_out.ensure_built((None, None, embedding_units))
    out_mlp.ensure_built((None, embedding_units) if output_embedding == "graph" else (None, None, embedding_units))
    layers = [embed_n, embed_e, dense0, adj_dense]
    for blk in blocks:
        layers += [blk["ln1"]] + blk["heads"] + [blk["merge"], blk["ln2"], blk["mlp"], blk["dense"]]
    layers += [ln_out, out_mlp]
    model = _MatModel(name, forward, layers,
                      config={"depth": depth, "heads": heads, "merge_heads": merge_heads,
                              "attention_kwargs": attention_kwargs, "distance_matrix_kwargs": distance_matrix_kwargs})
    model.__kgcnn_model_version__ = __model_version__
    model.attention_heads = [head for blk in blocks for head in blk["heads"]]
    model.attention_blocks = [blk["fused"] for blk in blocks]
    model.fused_attention_blocks = [bool(blk["fused"].supported()) for blk in blocks]
    model.auto_graph = True   # re-bound inputs replay the whole call sequence from one HIP graph (model/utils.py)
    return model
