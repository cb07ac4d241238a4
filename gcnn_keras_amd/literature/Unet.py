"""Graph U-Net model builder (mirror of kgcnn/literature/Unet.py:22-164, ``make_model``; Gao & Ji, arXiv:1905.05178).

``depth`` levels down - a mean-aggregating convolution, optionally the reconnect ``A^2`` (``AdjacencyPower``), then
``PoolingTopK`` - and ``depth`` levels up - ``UnPoolingTopK``, the skip connection, the same convolution - on the layers
of layers/pool/topk.py, whose kernels (csrc/mp_topk.hip) keep the batch ragged and dense-free at every level.

The convolution ``GatherNodesOutgoing -> Dense -> PoolingLocalEdges -> Activation`` runs its ``Dense`` on the ``N`` node
rows in front of the gather instead of on the ``M`` gathered edge rows: a Dense is row-wise and ``mp_dense_f32`` sums a
row's products in an order that does not depend on where the row stands, so the bits are those of the edge-side order
(tests/test_gpu_unet.py compares the two orders bit for bit).  The convolution has no self term: two nodes with the same
neighbour set carry bit-equal rows, hence equal scores - ``PoolingTopK``'s tie rule is in use on ordinary batches.

Up path: ``UnPoolingTopK`` and the ``LazyAdd`` of the skip connection are one launch (``call_with_skip``).  The edge
output of the reference's un-pooling is not computed: no layer behind it reads it, and with ``use_reconnect`` the
reference scatters positions of the ``A^2`` list into a tensor shaped like the list before ``A^2``, which has no defined
result.

The edge values reach ``AdjacencyPower`` and the pooled edge lists only; the model output depends on them through the
thresholded structure alone, so they are taken off the tape (their gradient is zero in the reference too) and an edge
embedding receives no gradient.

The sizes of every level depend on the data (one host read per ``AdjacencyPower`` and per ``PoolingTopK``), so the call
sequence cannot be captured into one HIP graph: ``auto_graph`` stays off for this model.

Weight order (``get_weights()``): node embedding, edge embedding (where the inputs are embedded), the input ``Dense``,
per level down the convolution's ``Dense`` and the pooling ``score``, per level up the convolution's ``Dense``, then the
output ``MLP``.
"""
from ..layers.casting import ChangeTensorType
from ..layers.gather import GatherNodesOutgoing
from ..layers.mlp import MLP, GraphMLP
from ..layers.modules import Activation, Dense, OptionalInputEmbedding
from ..layers.pool.topk import AdjacencyPower, PoolingTopK, UnPoolingTopK
from ..layers.pooling import PoolingLocalEdges, PoolingNodes
from ..model.utils import Model, update_model_kwargs

__model_version__ = "2022.11.25"

model_default = {
    "name": "Unet",
    "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None,), "name": "edge_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64},
                        "edge": {"input_dim": 5, "output_dim": 64}},
    "hidden_dim": {"units": 32, "use_bias": True, "activation": "linear"},
    "top_k_args": {"k": 0.3, "kernel_initializer": "ones"},
    "activation": "relu",
    "use_reconnect": True,
    "depth": 4,
    "pooling_args": {"pooling_method": "segment_mean"},
    "gather_args": {"node_indexing": "sample"},
    "verbose": 10,
    "output_embedding": "graph", "output_to_tensor": True,
    "output_mlp": {"use_bias": [True, False], "units": [25, 1], "activation": ["relu", "sigmoid"]}
}


@update_model_kwargs(model_default)
def make_model(inputs: list = None, input_embedding: dict = None, pooling_args: dict = None, gather_args: dict = None,
               top_k_args: dict = None, depth: int = None, use_reconnect: bool = None, hidden_dim: dict = None,
               activation: str = None, name: str = None, verbose: int = None, output_embedding: str = None,
               output_to_tensor: bool = None, output_mlp: dict = None):
    r"""Build Graph U-Net (kgcnn/literature/Unet.py:92-164).  Model inputs ``[node_attributes, edge_attributes,
    edge_indices]``, all ragged; ``output_embedding`` ``"graph"`` gives ``(batch, L)``, ``"node"`` the per-node output
    (a padded tensor with ``output_to_tensor``).  Column 0 of the edge attributes (of their embedding) is the adjacency
    weight of the reconnect step.  ``auto_graph`` is off: the level sizes are data dependent (module docstring)."""
    if output_embedding not in ("graph", "node"):
        raise ValueError("Unsupported graph embedding for mode `Unet`")
    embed_n = OptionalInputEmbedding(**input_embedding["node"], use_embedding=len(inputs[0]["shape"]) < 2)
    embed_e = OptionalInputEmbedding(**input_embedding["edge"], use_embedding=len(inputs[1]["shape"]) < 2)
    dense0 = Dense(**hidden_dim)
    down = [{"dense": Dense(**hidden_dim), "gather": GatherNodesOutgoing(**gather_args),
             "pool": PoolingLocalEdges(**pooling_args), "act": Activation(activation=activation),
             "power": AdjacencyPower(n=2) if use_reconnect else None, "topk": PoolingTopK(**top_k_args)}
            for _ in range(depth)]
    up = [{"unpool": UnPoolingTopK(), "dense": Dense(**hidden_dim), "gather": GatherNodesOutgoing(**gather_args),
           "pool": PoolingLocalEdges(**pooling_args), "act": Activation(activation=activation)} for _ in range(depth)]
    if output_embedding == "graph":
        pool_out, out_mlp, cast = PoolingNodes(**pooling_args), MLP(**output_mlp), None
    else:
        pool_out, out_mlp = None, GraphMLP(**output_mlp)
        cast = ChangeTensorType(input_tensor_type="ragged", output_tensor_type="tensor") if output_to_tensor else None

    def conv(lay, n, edi):
        # GatherNodesOutgoing -> Dense -> PoolingLocalEdges -> Activation, the Dense on the node rows (module docstring)
        eu = lay["gather"]([lay["dense"](n), edi])
        return lay["act"](lay["pool"]([n, eu, edi]))

    def forward(model_inputs, **kwargs):
        node_input, edge_input, edi = model_inputs
        n = dense0(embed_n(node_input))
        ed = embed_e(edge_input)
        ed = ed.with_values(ed.values.detach())   # structure only: the output has no gradient in the edge values
        graph_list, map_list = [[n, ed, edi]], []
        i_graph = graph_list[0]
        for lay in down:
            n, ed, edi = i_graph
            n = conv(lay, n, edi)
            if lay["power"] is not None:
                ed, edi = lay["power"]([n, ed, edi])
            i_graph, i_map = lay["topk"]([n, ed, edi])
            graph_list.append(i_graph)
            map_list.append(i_map)
        ui_graph = i_graph
        for i, lay in zip(range(depth, 0, -1), up):
            o_graph = graph_list[i - 1]
            n, ed, edi = lay["unpool"].call_with_skip(o_graph + map_list[i - 1] + ui_graph, o_graph[0], with_edges=False)
            ui_graph = [conv(lay, n, edi), ed, edi]
        n = ui_graph[0]
        if output_embedding == "graph":
            return out_mlp(pool_out(n))
        out = out_mlp(n)
        return cast(out) if cast is not None else out

    units = int(hidden_dim["units"])
    node_width = input_embedding["node"]["output_dim"] if len(inputs[0]["shape"]) < 2 else inputs[0]["shape"][-1]
    edge_width = input_embedding["edge"]["output_dim"] if len(inputs[1]["shape"]) < 2 else inputs[1]["shape"][-1]
    embed_n.ensure_built((None, None))
    embed_e.ensure_built((None, None))
    dense0.ensure_built((None, None, node_width))
    for lay in down:
        lay["dense"].ensure_built((None, None, units))
        lay["topk"].ensure_built([(None, None, units), (None, None, 1 if use_reconnect else edge_width), (None, None, 2)])
    for lay in up:
        lay["dense"].ensure_built((None, None, units))
    out_mlp.ensure_built((None, units) if output_embedding == "graph" else (None, None, units))
    layers = [embed_n, embed_e, dense0]
    for lay in down:
        layers += [lay["dense"], lay["gather"], lay["pool"], lay["act"]] + ([lay["power"]] if use_reconnect else []) \
            + [lay["topk"]]
    for lay in up:
        layers += [lay["unpool"], lay["dense"], lay["gather"], lay["pool"], lay["act"]]
    layers += ([pool_out] if pool_out is not None else []) + [out_mlp] + ([cast] if cast is not None else [])
    model = Model(name, forward, layers,
                  config={"depth": depth, "use_reconnect": use_reconnect, "top_k_args": top_k_args,
                          "hidden_dim": hidden_dim, "output_embedding": output_embedding,
                          "edge_input_dim": input_embedding["edge"]["input_dim"] if embed_e.use_embedding else None})
    model.__kgcnn_model_version__ = __model_version__
    model.pooling_layers = [lay["topk"] for lay in down]
    return model
