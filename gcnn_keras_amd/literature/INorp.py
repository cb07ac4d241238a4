"""INorp model builder (mirror of kgcnn/literature/INorp.py:23-153, ``make_model``): Interaction Networks
(Battaglia et al., https://arxiv.org/abs/1612.00222).

Per block an edge MLP reads ``[n_outgoing || n_ingoing || e]``, its output is pooled at the receiver, and a node MLP reads
``[n || pooled || graph state]``; the graph state is gathered to the nodes once, in front of the blocks.  The readout is a
node pool (or ``Dense`` + ``PoolingSet2Set``) and an MLP, or a per-node MLP.

The edge side of a block is one ``INorpEdgeStep`` (``layers/conv/inorp_conv.py``) around the block's edge ``GraphMLP``
and ``PoolingLocalEdges``.  By default a step runs the layer sequence, the reference's ops.  With
``model.use_fused_step = True`` (or ``step.use_fused_step``) the blocks whose edge MLP is ``Dense(H1, act) -> Dense(H2,
linear)`` with served sizes take the fused route (csrc/mp_inorp.hip: the second Dense moves behind the pool, no edge-sized
tensor is written), with and without a tape: ``compile`` / ``train_on_batch`` / ``fit`` then record
``autograd.InorpEdge``.  ``model.fused_step_rounds`` counts the blocks the fused route serves (0 for the default
dictionary's five-layer edge MLP).  The switch is off by default: on 128 molecule graphs the fused route issued fewer engine
calls and was faster eager, but slower replayed from a HIP graph and in a training step.  With
``use_set2set=True`` training raises ``NotImplementedError`` from ``PoolingSet2Set``, which has no LSTM reverse.
"""
from ..layers.casting import ChangeTensorType
from ..layers.conv.inorp_conv import INorpEdgeStep
from ..layers.gather import GatherState
from ..layers.mlp import MLP, GraphMLP
from ..layers.modules import Dense, LazyConcatenate, OptionalInputEmbedding
from ..layers.pool.set2set import PoolingSet2Set
from ..layers.pooling import PoolingLocalEdges, PoolingNodes
from ..model.utils import RouteSwitchModel, update_model_kwargs
from ..ragged import RaggedTensor

__model_version__ = "2022.11.25"

hyper_model_default = {
    "name": "INorp",
    "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None,), "name": "edge_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": [], "name": "graph_attributes", "dtype": "float32", "ragged": False}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64},
                        "edge": {"input_dim": 5, "output_dim": 64},
                        "graph": {"input_dim": 100, "output_dim": 64}},
    "set2set_args": {"channels": 32, "T": 3, "pooling_method": "mean", "init_qstar": "mean"},
    "node_mlp_args": {"units": [100, 50], "use_bias": True, "activation": ["relu", "linear"]},
    "edge_mlp_args": {"units": [100, 100, 100, 100, 50],
                      "activation": ["relu", "relu", "relu", "relu", "linear"]},
    "pooling_args": {"pooling_method": "segment_mean"},
    "depth": 3, "use_set2set": False, "verbose": 10,
    "gather_args": {},
    "output_embedding": "graph", "output_to_tensor": True,
    "output_mlp": {"use_bias": [True, True, False], "units": [25, 10, 1],
                   "activation": ["relu", "relu", "sigmoid"]}
}
model_default = hyper_model_default


class _INorpModel(RouteSwitchModel):
    """``Model`` with the ``use_fused_step`` switch over all blocks."""

    switch_attr, switch_layers_attr = "use_fused_step", "step_layers"
    step_layers = ()
    use_fused_step = RouteSwitchModel.switch


def _last(args):
    return args["units"][-1] if isinstance(args["units"], (list, tuple)) else args["units"]


@update_model_kwargs(hyper_model_default)
def make_model(inputs: list = None, input_embedding: dict = None, depth: int = None, gather_args: dict = None,
               edge_mlp_args: dict = None, node_mlp_args: dict = None, set2set_args: dict = None,
               pooling_args: dict = None, use_set2set: dict = None, name: str = None, verbose: int = None,
               output_embedding: str = None, output_to_tensor: bool = None, output_mlp: dict = None):
    r"""Build INorp (kgcnn/literature/INorp.py:99-153).  Model inputs ``[node_attributes, edge_attributes, edge_indices,
    graph_attributes]``: nodes ``(batch, None, F)`` or ``(batch, None)`` through an embedding, edges likewise, the graph
    state ``(batch, F)`` or ``(batch,)`` through an embedding.  Output ``(batch, L)`` for ``output_embedding="graph"``,
    per node for ``"node"``."""
    if output_embedding not in ("graph", "node"):
        raise ValueError("Unsupported output embedding for mode `INorp`")
    embed_n = OptionalInputEmbedding(**input_embedding["node"], use_embedding=len(inputs[0]["shape"]) < 2)
    embed_e = OptionalInputEmbedding(**input_embedding["edge"], use_embedding=len(inputs[1]["shape"]) < 2)
    embed_u = OptionalInputEmbedding(**input_embedding["graph"], use_embedding=len(inputs[3]["shape"]) < 1)
    gather_state = GatherState(**gather_args)
    edge_mlps = [GraphMLP(**edge_mlp_args) for _ in range(depth)]
    node_mlps = [GraphMLP(**node_mlp_args) for _ in range(depth)]
    steps = [INorpEdgeStep(mlp=edge_mlps[i], pooling=PoolingLocalEdges(**pooling_args), gather_args=gather_args)
             for i in range(depth)]                          # around the block's layers: a step owns no weight
    concats = [LazyConcatenate(axis=-1) for _ in range(depth)]
    graph_out = output_embedding == "graph"
    dense_s2s = Dense(set2set_args["channels"], activation="linear") if (graph_out and use_set2set) else None
    if graph_out:
        readout = PoolingSet2Set(**set2set_args) if use_set2set else PoolingNodes(**pooling_args)
        out_mlp = MLP(**output_mlp)
    else:
        readout = None
        out_mlp = GraphMLP(**output_mlp)
    cast = ChangeTensorType(input_tensor_type="ragged", output_tensor_type="tensor") \
        if (not graph_out and output_to_tensor) else None

    def forward(model_inputs, **kwargs):
        node_input, edge_input, edi, env_input = model_inputs
        for x in model_inputs:
            # the per-graph pools read the host copy of the splits: taken once from the inputs, every derived tensor
            # inherits it and the call sequence can be captured
            if isinstance(x, RaggedTensor):
                x.row_splits_host()
        n, ed, uenv = embed_n(node_input), embed_e(edge_input), embed_u(env_input)
        ev = gather_state([uenv, n])
        for i in range(depth):
            nu = steps[i]([n, ed, edi])
            n = node_mlps[i](concats[i]([n, nu, ev]))
        if graph_out:
            out = readout(dense_s2s(n)) if use_set2set else readout(n)
            return out_mlp(out.reshape(int(out.shape[0]), -1).contiguous())    # ks.layers.Flatten
        out = out_mlp(n)
        return cast(out) if cast is not None else out

    # weights in the reference's construction order, so set_weights() works before a first call
    node_dim = input_embedding["node"]["output_dim"] if len(inputs[0]["shape"]) < 2 else inputs[0]["shape"][-1]
    edge_dim = input_embedding["edge"]["output_dim"] if len(inputs[1]["shape"]) < 2 else inputs[1]["shape"][-1]
    env_dim = input_embedding["graph"]["output_dim"] if len(inputs[3]["shape"]) < 1 else inputs[3]["shape"][-1]
    embed_n.ensure_built((None, None))
    embed_e.ensure_built((None, None))
    embed_u.ensure_built((None,))
    layers = [embed_n, embed_e, embed_u]
    width = node_dim
    for i in range(depth):
        steps[i].ensure_built([(None, None, width), (None, None, edge_dim), (None, None, 2)])   # builds the edge MLP
        node_mlps[i].ensure_built((None, None, width + _last(edge_mlp_args) + env_dim))
        layers += [edge_mlps[i], node_mlps[i]]
        width = _last(node_mlp_args)
    if dense_s2s is not None:
        dense_s2s.ensure_built((None, None, width))
        readout.ensure_built((None, None, set2set_args["channels"]))
        layers += [dense_s2s, readout]
        width = 2 * set2set_args["channels"]
    out_mlp.ensure_built((None, width) if graph_out else (None, None, width))
    layers.append(out_mlp)
    model = _INorpModel(name, forward, layers,
                        config={"inputs": inputs, "input_embedding": input_embedding, "depth": depth,
                                "edge_mlp_args": edge_mlp_args, "node_mlp_args": node_mlp_args,
                                "set2set_args": set2set_args, "pooling_args": pooling_args, "use_set2set": use_set2set,
                                "output_embedding": output_embedding, "output_mlp": output_mlp})
    model.__kgcnn_model_version__ = __model_version__
    model.step_layers = steps
    model.fused_step_rounds = sum(bool(lay.fused_step) for lay in steps)   # how many blocks the fused route serves
    # re-bound inputs replay the whole forward from one HIP graph (model/utils.py); the route is part of its identity
    model.auto_graph = True
    return model
