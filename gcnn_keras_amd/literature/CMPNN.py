"""CMPNN model builder (mirror of kgcnn/literature/CMPNN.py:23-174, ``make_model``): communicative message passing
(Song et al. 2020, https://www.ijcai.org/proceedings/2020/0392.pdf).

Nodes and directed edges both carry a state.  Each of ``depth - 1`` rounds first boosts the nodes,
``h += pool(he) * max(he)`` over the incoming edges, then updates every edge from its sender's new state minus the state of
its reverse edge, ``he = act(Dense(h[j] - he[reverse]) + he0)``, with a ``Dense`` of its own per round.  A last booster's
product is concatenated with ``h`` and the initial ``h0`` into ``Dense(**node_dense)``; the readout is a GRU over each
graph's node sequence (``layers/pool/gru.py``) or ``PoolingNodes``.

A round is one ``CMPNNCommunicate`` (``layers/conv/cmpnn_conv.py``).  Rounds whose sizes fit run on the two fused kernels of
csrc/mp_cmpnn.hip outside a tape; ``model.fused_communicate_rounds`` lists which do, ``model.use_fused_communicate`` (or
``round.use_fused_communicate``) switches the route.  ``Dropout`` is the identity at inference.  Training is not built: max
pooling has no reverse rule and the GRU readout is forward only, so a call in grad mode with trainable weights raises
``NotImplementedError``.
"""
from ..layers.casting import ChangeTensorType
from ..layers.conv.cmpnn_conv import CMPNNBoost, CMPNNCommunicate
from ..layers.mlp import MLP, GraphMLP
from ..layers.modules import Dense, LazyConcatenate, OptionalInputEmbedding
from ..layers.pool.gru import PoolingNodesGRU
from ..layers.pooling import PoolingNodes
from ..model.utils import RouteSwitchModel, update_model_kwargs

__model_version__ = "2022.11.25"

model_default = {
    "name": "CMPNN",
    "inputs": [
        {"shape": (None,), "name": "node_number", "dtype": "float32", "ragged": True},
        {"shape": (None,), "name": "edge_attributes", "dtype": "float32", "ragged": True},
        {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
        {"shape": (None, 1), "name": "edge_indices_reverse", "dtype": "int64", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64},
                        "edge": {"input_dim": 5, "output_dim": 64}},
    "node_initialize": {"units": 300, "activation": "relu"},
    "edge_initialize": {"units": 300, "activation": "relu"},
    "edge_dense": {"units": 300, "activation": "linear"},
    "node_dense": {"units": 300, "activation": "linear"},
    "edge_activation": {"activation": "relu"},
    "verbose": 10,
    "depth": 5,
    "dropout": {"rate": 0.1},
    "use_final_gru": True,
    "pooling_gru": {"units": 300},
    "pooling_kwargs": {"pooling_method": "sum"},
    "output_embedding": "graph", "output_to_tensor": True,
    "output_mlp": {"use_bias": [True, True, False], "units": [300, 100, 1],
                   "activation": ["relu", "relu", "linear"]}
}


class _CmpnnModel(RouteSwitchModel):
    """``Model`` with the ``use_fused_communicate`` switch over all rounds and the last booster."""

    switch_attr, switch_layers_attr = "use_fused_communicate", "communicate_layers"
    communicate_layers = ()
    use_fused_communicate = RouteSwitchModel.switch


def _width(spec, embedding):
    return embedding["output_dim"] if len(spec["shape"]) < 2 else spec["shape"][-1]


@update_model_kwargs(model_default)
def make_model(name: str = None, inputs: list = None, input_embedding: dict = None, edge_initialize: dict = None,
               node_initialize: dict = None, edge_dense: dict = None, node_dense: dict = None,
               edge_activation: dict = None, depth: int = None, dropout: dict = None, verbose: int = None,
               use_final_gru: bool = True, pooling_gru: dict = None, pooling_kwargs: dict = None,
               output_embedding: str = None, output_to_tensor: bool = None, output_mlp: dict = None):
    r"""Build CMPNN (kgcnn/literature/CMPNN.py:109-174).  Model inputs ``[node_attributes, edge_attributes, edge_indices,
    edge_indices_reverse]``: nodes and edges as integer types ``(batch, [N])`` for the embeddings or as features
    ``(batch, [N], F)``; the last input holds, per edge, the position of its reverse edge in the graph's edge list (``-1`` if
    there is none).  Output: ``(batch, L)`` for ``output_embedding="graph"``, per node for ``"node"``."""
    if output_embedding not in ("graph", "node"):
        raise ValueError("Unsupported graph embedding for mode `CMPNN`")
    embed_n = OptionalInputEmbedding(**input_embedding["node"], use_embedding=len(inputs[0]["shape"]) < 2)
    embed_e = OptionalInputEmbedding(**input_embedding["edge"], use_embedding=len(inputs[1]["shape"]) < 2)
    dense_h0 = Dense(**node_initialize)
    dense_he0 = Dense(**edge_initialize)
    # a new Dense(**edge_dense) in every round (the reference creates the layer inside its loop)
    rounds = [CMPNNCommunicate(edge_dense=edge_dense, edge_activation=edge_activation, pooling_kwargs=pooling_kwargs,
                               dropout=dropout) for _ in range(depth - 1)]
    last_boost = CMPNNBoost(**pooling_kwargs, m_only=True)
    concat = LazyConcatenate(axis=-1)
    dense_node = Dense(**node_dense)
    readout = None
    if output_embedding == "graph":
        readout = PoolingNodesGRU(**pooling_gru) if use_final_gru else PoolingNodes(**pooling_kwargs)
        out_mlp = MLP(**output_mlp)
    else:
        out_mlp = GraphMLP(**output_mlp)
    cast = ChangeTensorType(input_tensor_type="ragged", output_tensor_type="tensor") \
        if (output_embedding == "node" and output_to_tensor) else None

    def forward(model_inputs, **kwargs):
        node_input, edge_input, edi, ed_pairs = model_inputs
        n, ed = embed_n(node_input), embed_e(edge_input)
        h0, he0 = dense_h0(n), dense_he0(ed)
        h, he = h0, he0
        for lay in rounds:
            h, he = lay([h, he, he0, edi, ed_pairs], **kwargs)
        m = last_boost([h, he, edi], **kwargs)
        h_final = dense_node(concat([m, h, h0]))
        if output_embedding == "graph":
            return out_mlp(readout(h_final))
        out = out_mlp(h_final)
        return cast(out) if cast is not None else out

    node_width, edge_width = _width(inputs[0], input_embedding["node"]), _width(inputs[1], input_embedding["edge"])
    fn, fe0 = node_initialize["units"], edge_initialize["units"]
    fe = fe0
    embed_n.ensure_built((None, None))
    embed_e.ensure_built((None, None))
    dense_h0.ensure_built((None, None, node_width))
    dense_he0.ensure_built((None, None, edge_width))
    for lay in rounds:
        lay.ensure_built([(None, None, fn), (None, None, fe), (None, None, fe0), (None, None, 2), (None, None, 1)])
        fe = lay.lay_dense.units
    last_boost.ensure_built([(None, None, fn), (None, None, fe), (None, None, 2)])
    dense_node.ensure_built((None, None, fe + 2 * fn))
    if isinstance(readout, PoolingNodesGRU):
        readout.ensure_built((None, None, node_dense["units"]))
        width = readout.units
    else:
        width = node_dense["units"]
    out_mlp.ensure_built((None, width) if output_embedding == "graph" else (None, None, width))
    layers = [embed_n, embed_e, dense_h0, dense_he0] + rounds + [last_boost, dense_node] + \
             ([readout] if readout is not None else []) + [out_mlp]
    model = _CmpnnModel(name, forward, layers,
                        config={"depth": depth, "node_initialize": node_initialize, "edge_initialize": edge_initialize,
                                "edge_dense": edge_dense, "node_dense": node_dense, "use_final_gru": use_final_gru,
                                "pooling_gru": pooling_gru, "pooling_kwargs": pooling_kwargs})
    model.__kgcnn_model_version__ = __model_version__
    model.communicate_layers = rounds + [last_boost]
    model.fused_communicate_rounds = [bool(lay.fused_communicate) for lay in rounds]
    # re-bound inputs replay the whole forward from one HIP graph (model/utils.py); the route is part of its identity
    model.auto_graph = True
    return model
