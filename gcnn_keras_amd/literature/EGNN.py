"""EGNN model builder (mirror of kgcnn/literature/EGNN.py:23-208): Satorras, Hoogeboom, Welling, "E(n) Equivariant Graph
Neural Networks" (https://arxiv.org/abs/2102.09844).

Per block: squared (or plain) distance of every edge, optionally its position encoding; the edge model on ``[h_i, h_j,
enc, (edge attributes)]`` with an optional one-unit attention gate; optionally the coordinate model (``x <- x + mean_j
(x_i - x_j) phi_x(m_ij)``); the node model on ``[h, sum_j m_ij, (h0)]`` with an optional skip.

The op sequence is the reference's, including its two quirks:

* ``expand_distance_kwargs`` only switches the position encoding on; the layer is built with its **defaults**
  (EGNN.py:151-152, ``PositionEncodingBasisLayer()``), so ``{"dim_half": 64}`` still gives 20 columns;
* the node decoder is built from ``node_mlp_kwargs``; ``node_decoder_kwargs`` only switches it on (EGNN.py:188-189).

A block whose sizes fit ``layers/conv/egnn_conv.py`` (width 128, a two-layer edge MLP of 128, no edge attributes, no
coordinate model, sum pooling) runs its edge step on the fused ``mp_egnn_edge_f32``; every other configuration, a call in
grad mode with trainable edge weights, and ``model.use_fused_edge = False`` take the layer sequence.
``node_normalize_kwargs`` raises ``NotImplementedError`` (``GraphLayerNormalization`` has no reverse pass).
"""
from ..layers.casting import ChangeTensorType
from ..layers.conv.egnn_conv import FusedEdgeStep, fused_edge_supported
from ..layers.gather import GatherEmbeddingSelection
from ..layers.geom import EdgeDirectionNormalized, EuclideanNorm, NodePosition, PositionEncodingBasisLayer
from ..layers.mlp import MLP, GraphMLP
from ..layers.modules import LazyAdd, LazyConcatenate, LazyMultiply, LazySubtract, OptionalInputEmbedding
from ..layers.pooling import PoolingLocalEdges, PoolingNodes
from ..model.utils import Model, update_model_kwargs

__model_version__ = "2022.11.25"

model_default = {
    "name": "EGNN",
    "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 3), "name": "node_coordinates", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": (None, 10), "name": "edge_attributes", "dtype": "float32", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64},
                        "edge": {"input_dim": 95, "output_dim": 64}},
    "depth": 4,
    "node_mlp_initialize": None,
    "euclidean_norm_kwargs": {"keepdims": True, "axis": 2},
    "use_edge_attributes": True,
    "edge_mlp_kwargs": {"units": [64, 64], "activation": ["swish", "linear"]},
    "edge_attention_kwargs": None,  # {"units: 1", "activation": "sigmoid"}
    "use_normalized_difference": False,
    "expand_distance_kwargs": None,
    "coord_mlp_kwargs": {"units": [64, 1], "activation": ["swish", "linear"]},  # option: "tanh" at the end.
    "pooling_coord_kwargs": {"pooling_method": "mean"},
    "pooling_edge_kwargs": {"pooling_method": "sum"},
    "node_normalize_kwargs": None,
    "use_node_attributes": False,
    "node_mlp_kwargs": {"units": [64, 64], "activation": ["swish", "linear"]},
    "use_skip": True,
    "verbose": 10,
    "node_decoder_kwargs": None,
    "node_pooling_kwargs": {"pooling_method": "sum"},
    "output_embedding": "graph",
    "output_to_tensor": True,
    "output_mlp": {"use_bias": [True, True], "units": [64, 1],
                   "activation": ["swish", "linear"]}
}


class _EgnnModel(Model):
    """``Model`` with the ``use_fused_edge`` switch: changing it drops the captured HIP graphs, which hold the route
    they were captured on."""

    _use_fused_edge = True

    @property
    def use_fused_edge(self):
        return self._use_fused_edge

    @use_fused_edge.setter
    def use_fused_edge(self, value):
        if bool(value) != self._use_fused_edge:
            self.release_graphs()
        self._use_fused_edge = bool(value)


def _last_units(mlp_kwargs):
    units = mlp_kwargs["units"]
    return units[-1] if isinstance(units, (list, tuple)) else units


@update_model_kwargs(model_default)
def make_model(name: str = None, inputs: list = None, input_embedding: dict = None, depth: int = None,
               euclidean_norm_kwargs: dict = None, node_mlp_initialize: dict = None, use_edge_attributes: bool = None,
               edge_mlp_kwargs: dict = None, edge_attention_kwargs: dict = None,
               use_normalized_difference: bool = None, expand_distance_kwargs: dict = None,
               coord_mlp_kwargs: dict = None, pooling_coord_kwargs: dict = None, pooling_edge_kwargs: dict = None,
               node_normalize_kwargs: dict = None, use_node_attributes: bool = None, node_mlp_kwargs: dict = None,
               use_skip: bool = None, verbose: int = None, node_decoder_kwargs: dict = None,
               node_pooling_kwargs: dict = None, output_embedding: str = None, output_to_tensor: bool = None,
               output_mlp: dict = None):
    r"""Build EGNN (kgcnn/literature/EGNN.py:56-208).  Model inputs ``[node_attributes, node_coordinates, edge_indices,
    edge_attributes]`` (the last may be left out with ``use_edge_attributes=False``); output ``(batch, L)`` graph
    embeddings or, with ``output_embedding="node"``, node embeddings.  See the module docstring for the two quirks of the
    reference that are kept (``expand_distance_kwargs`` and ``node_decoder_kwargs`` are switches only)."""
    if output_embedding not in ("graph", "node"):
        raise ValueError("Unsupported output embedding for mode `EGNN`")
    if node_normalize_kwargs:
        raise NotImplementedError("EGNN with node_normalize_kwargs: GraphLayerNormalization has no reverse pass here")
    embed_e = OptionalInputEmbedding(**input_embedding["edge"], use_embedding=len(inputs[3]["shape"]) < 2)
    embed_n = OptionalInputEmbedding(**input_embedding["node"], use_embedding=len(inputs[0]["shape"]) < 2)
    mlp_init = GraphMLP(**node_mlp_initialize) if node_mlp_initialize else None
    lay_pos, lay_sub, lay_norm = NodePosition(), LazySubtract(), EuclideanNorm(**euclidean_norm_kwargs)
    lay_dir = EdgeDirectionNormalized() if use_normalized_difference else None
    lay_gather = GatherEmbeddingSelection([0, 1])
    lay_cat, lay_mul, lay_add = LazyConcatenate(), LazyMultiply(), LazyAdd()
    lay_pool_x = PoolingLocalEdges(**pooling_coord_kwargs) if coord_mlp_kwargs else None
    lay_pool_e = PoolingLocalEdges(**pooling_edge_kwargs)
    encodings, edge_mlps, att_mlps, coord_mlps, node_mlps = [], [], [], [], []
    for _ in range(depth):
        # the reference builds the encoding with its defaults whatever expand_distance_kwargs holds (EGNN.py:151-152)
        encodings.append(PositionEncodingBasisLayer() if expand_distance_kwargs else None)
        edge_mlps.append(GraphMLP(**edge_mlp_kwargs) if edge_mlp_kwargs else None)
        att_mlps.append(GraphMLP(**edge_attention_kwargs) if edge_attention_kwargs else None)
        coord_mlps.append(GraphMLP(**coord_mlp_kwargs) if coord_mlp_kwargs else None)
        node_mlps.append(GraphMLP(**node_mlp_kwargs) if node_mlp_kwargs else None)
    # the decoder takes node_mlp_kwargs (EGNN.py:188-189)
    decoder = GraphMLP(**node_mlp_kwargs) if node_decoder_kwargs else None
    pool = PoolingNodes(**node_pooling_kwargs) if output_embedding == "graph" else None
    out_mlp = MLP(**output_mlp) if output_embedding == "graph" else GraphMLP(**output_mlp)
    cast = ChangeTensorType(input_tensor_type="ragged", output_tensor_type="tensor") \
        if (output_embedding == "node" and output_to_tensor) else None

    # weights exist before the first call (set_weights / get_weights); widths follow the op sequence
    h0_dim = input_embedding["node"]["output_dim"] if embed_n.use_embedding else inputs[0]["shape"][-1]
    ed_dim = input_embedding["edge"]["output_dim"] if embed_e.use_embedding else inputs[3]["shape"][-1]
    embed_e.ensure_built((None, None))
    embed_n.ensure_built((None, None))
    hw = h0_dim
    if mlp_init is not None:
        mlp_init.ensure_built((None, None, h0_dim))
        hw = _last_units(node_mlp_initialize)
    steps = []
    for i in range(depth):
        norm_dim = 2 * encodings[i].dim_half if encodings[i] is not None else 1
        mw = 2 * hw + norm_dim + (ed_dim if use_edge_attributes else 0)
        fits = (not use_edge_attributes and not coord_mlp_kwargs and bool(euclidean_norm_kwargs.get("keepdims"))
                and fused_edge_supported(hw, edge_mlps[i], att_mlps[i], encodings[i], lay_pool_e.pooling_method,
                                         lay_pool_e.pooling_index))
        steps.append(FusedEdgeStep(edge_mlps[i], att_mlps[i], encodings[i]) if fits else None)
        if edge_mlps[i] is not None:
            edge_mlps[i].ensure_built((None, None, mw))
            mw = _last_units(edge_mlp_kwargs)
        if att_mlps[i] is not None:
            att_mlps[i].ensure_built((None, None, mw))
        if coord_mlps[i] is not None:
            coord_mlps[i].ensure_built((None, None, mw))
        if node_mlps[i] is not None:
            node_mlps[i].ensure_built((None, None, hw + mw + (h0_dim if use_node_attributes else 0)))
            mw = _last_units(node_mlp_kwargs)
        if not use_skip:
            hw = mw
    if decoder is not None:
        decoder.ensure_built((None, None, hw))
        hw = _last_units(node_mlp_kwargs)
    out_mlp.ensure_built((None, hw) if output_embedding == "graph" else (None, None, hw))

    def edge_step(i, h, norm_x, ed, edi, **kwargs):
        """``(m_ij or None, m_i)`` of block ``i``: fused when the block fits and its weights are frozen."""
        step = steps[i]
        if step is not None and model.use_fused_edge and not step.weights_need_grad():
            return None, step(h, norm_x, edi)
        if encodings[i] is not None:
            norm_x = encodings[i](norm_x, **kwargs)
        h_i, h_j = lay_gather([h, edi], **kwargs)
        m_ij = lay_cat([h_i, h_j, norm_x, ed] if use_edge_attributes else [h_i, h_j, norm_x], **kwargs)
        if edge_mlps[i] is not None:
            m_ij = edge_mlps[i](m_ij, **kwargs)
        if att_mlps[i] is not None:
            m_att = att_mlps[i](m_ij, **kwargs)
            m_ij = lay_mul([m_att, m_ij], **kwargs)
        return m_ij, None

    def forward(model_inputs, **kwargs):
        node_input, xyz_input, edi = model_inputs[:3]
        if use_edge_attributes and len(model_inputs) < 4:
            raise ValueError("EGNN with use_edge_attributes expects [node_attributes, node_coordinates, edge_indices, "
                             "edge_attributes]")
        ed = embed_e(model_inputs[3]) if use_edge_attributes else None
        h0 = embed_n(node_input)
        h = mlp_init(h0, **kwargs) if mlp_init is not None else h0
        x = xyz_input
        for i in range(depth):
            pos1, pos2 = lay_pos([x, edi], **kwargs)
            diff_x = lay_sub([pos1, pos2], **kwargs)
            norm_x = lay_norm(diff_x, **kwargs)
            if lay_dir is not None:
                diff_x = lay_dir([pos1, pos2], **kwargs)
            m_ij, m_i = edge_step(i, h, norm_x, ed, edi, **kwargs)
            if coord_mlps[i] is not None:
                m_ij_weights = coord_mlps[i](m_ij, **kwargs)
                x_trans = lay_mul([m_ij_weights, diff_x], **kwargs)
                agg = lay_pool_x([h, x_trans, edi], **kwargs)
                x = lay_add([x, agg], **kwargs)
            if m_i is None:
                m_i = lay_pool_e([h, m_ij, edi], **kwargs)
            if node_mlps[i] is not None:
                m_i = lay_cat([h, m_i], **kwargs)
                if use_node_attributes:
                    m_i = lay_cat([m_i, h0], **kwargs)
                m_i = node_mlps[i](m_i, **kwargs)
            h = lay_add([h, m_i], **kwargs) if use_skip else m_i
        n = decoder(h, **kwargs) if decoder is not None else h
        if output_embedding == "graph":
            return out_mlp(pool(n, **kwargs), **kwargs)
        out = out_mlp(n, **kwargs)
        return cast(out) if cast is not None else out

    layers = [embed_e, embed_n] + ([mlp_init] if mlp_init is not None else [])
    for i in range(depth):
        layers += [lay for lay in (encodings[i], edge_mlps[i], att_mlps[i], coord_mlps[i], node_mlps[i])
                   if lay is not None]
    layers += ([decoder] if decoder is not None else []) + [out_mlp]
    config = {"inputs": inputs, "input_embedding": input_embedding, "depth": depth,
              "euclidean_norm_kwargs": euclidean_norm_kwargs, "node_mlp_initialize": node_mlp_initialize,
              "use_edge_attributes": use_edge_attributes, "edge_mlp_kwargs": edge_mlp_kwargs,
              "edge_attention_kwargs": edge_attention_kwargs, "use_normalized_difference": use_normalized_difference,
              "expand_distance_kwargs": expand_distance_kwargs, "coord_mlp_kwargs": coord_mlp_kwargs,
              "pooling_coord_kwargs": pooling_coord_kwargs, "pooling_edge_kwargs": pooling_edge_kwargs,
              "node_normalize_kwargs": node_normalize_kwargs, "use_node_attributes": use_node_attributes,
              "node_mlp_kwargs": node_mlp_kwargs, "use_skip": use_skip, "node_decoder_kwargs": node_decoder_kwargs,
              "node_pooling_kwargs": node_pooling_kwargs, "output_embedding": output_embedding,
              "output_to_tensor": output_to_tensor, "output_mlp": output_mlp}
    model = _EgnnModel(name, forward, layers, config=config)
    model.__kgcnn_model_version__ = __model_version__
    model.fused = None
    model.use_fused_edge = True             # False: every block takes the reference's layer sequence
    model.fused_edge_blocks = [s is not None for s in steps]
    model.edge_step = edge_step             # (i, h, norm_x, ed, edi) -> (m_ij, None) or (None, m_i): tests, benchmarks
    # the layer sequence is replayed from one HIP graph for re-bound inputs (model/utils.py)
    model.auto_graph = True
    return model
