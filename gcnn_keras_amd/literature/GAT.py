"""GAT model builder (mirror of kgcnn/literature/GAT.py:20-123, ``make_model``) on the engine's attention heads.

Each block's heads are handed to one ``FusedAttentionBlock`` (layers/conv/gat_conv.py): where the sizes fit
(``model.fused_attention_blocks``) the block runs on csrc/mp_gat.hip, three node-side Dense launches per head plus two
launches for all heads; every other configuration, every call on a tape (training) and ``model.use_fused_attention =
False`` take the layer sequence, one engine call per Keras layer."""
from ..layers.casting import ChangeTensorType
from ..layers.conv.gat_conv import AttentionHeadGAT, FusedAttentionBlock
from ..layers.mlp import MLP, GraphMLP
from ..layers.modules import Activation, Dense, LazyAverage, LazyConcatenate, OptionalInputEmbedding
from ..layers.pooling import PoolingNodes
from ..model.utils import RouteSwitchModel, update_model_kwargs

__model_version__ = "2022.11.25"

model_default = {
    "name": "GAT",
    "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None,), "name": "edge_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64},
                        "edge": {"input_dim": 5, "output_dim": 64}},
    "attention_args": {"units": 32, "use_final_activation": False, "use_edge_features": True,
                       "has_self_loops": True, "activation": "kgcnn>leaky_relu", "use_bias": True},
    "pooling_nodes_args": {"pooling_method": "mean"},
    "depth": 3, "attention_heads_num": 5,
    "attention_heads_concat": False, "verbose": 10,
    "output_embedding": "graph", "output_to_tensor": True,
    "output_mlp": {"use_bias": [True, True, False], "units": [25, 10, 1],
                   "activation": ["relu", "relu", "sigmoid"]}
}


class _GatModel(RouteSwitchModel):
    """``Model`` with the ``use_fused_attention`` switch over all heads."""

    switch_attr, switch_layers_attr = "use_fused_attention", "attention_heads"
    attention_heads = ()
    use_fused_attention = RouteSwitchModel.switch


def _feature_width(spec, embedding):
    return embedding["output_dim"] if len(spec["shape"]) < 2 else spec["shape"][-1]


@update_model_kwargs(model_default)
def make_model(inputs: list = None, input_embedding: dict = None, attention_args: dict = None,
               pooling_nodes_args: dict = None, depth: int = None, attention_heads_num: int = None,
               attention_heads_concat: bool = None, name: str = None, verbose: int = None,
               output_embedding: str = None, output_to_tensor: bool = None, output_mlp: dict = None,
               head_class=AttentionHeadGAT):
    r"""Build GAT (kgcnn/literature/GAT.py:89-121).  Model inputs ``[node_attributes, edge_attributes, edge_indices]``;
    per block ``attention_heads_num`` heads are concatenated or averaged (then activated).  ``head_class`` lets the
    GATv2 builder reuse this wiring.  ``model.fused_attention_blocks`` lists which blocks fit the fused kernels;
    ``model.attention_heads[i].use_fused_attention`` / ``model.use_fused_attention`` switch the route."""
    if output_embedding not in ("graph", "node"):
        raise ValueError("Unsupported output embedding for `GAT`")
    embed_n = OptionalInputEmbedding(**input_embedding["node"], use_embedding=len(inputs[0]["shape"]) < 2)
    embed_e = OptionalInputEmbedding(**input_embedding["edge"], use_embedding=len(inputs[1]["shape"]) < 2)
    units = attention_args["units"]
    dense0 = Dense(units=units, activation="linear")
    heads = [[head_class(**attention_args) for _ in range(attention_heads_num)] for _ in range(depth)]
    blocks = [FusedAttentionBlock(block) for block in heads]
    combine = LazyConcatenate(axis=-1) if attention_heads_concat else LazyAverage()
    head_act = None if attention_heads_concat else Activation(activation=attention_args["activation"])
    pool = PoolingNodes(**pooling_nodes_args) if output_embedding == "graph" else None
    out_mlp = MLP(**output_mlp) if output_embedding == "graph" else GraphMLP(**output_mlp)
    cast = ChangeTensorType(input_tensor_type="ragged", output_tensor_type="tensor") \
        if (output_embedding == "node" and output_to_tensor) else None

    def forward(model_inputs, **kwargs):
        node_input, edge_input, edi = model_inputs
        nk = dense0(embed_n(node_input))
        ed = embed_e(edge_input)
        for block, fused in zip(heads, blocks):
            if fused.route(nk, ed, None):
                stacked, _ = fused(nk, ed, edi)
                n, k, u = stacked.shape
                if attention_heads_concat:      # the concatenated heads are the tensor itself
                    nk = nk.with_values(stacked.view(n, k * u))
                else:
                    nk = combine([nk.with_values(stacked[:, i]) for i in range(k)])
            else:
                nk = combine([head([nk, ed, edi]) for head in block])
            if head_act is not None:
                nk = head_act(nk)
        if output_embedding == "graph":
            return out_mlp(pool(nk))
        out = out_mlp(nk)
        return cast(out) if cast is not None else out

    node_width = _feature_width(inputs[0], input_embedding["node"])
    edge_width = _feature_width(inputs[1], input_embedding["edge"])
    embed_n.ensure_built((None, None))
    embed_e.ensure_built((None, None))
    dense0.ensure_built((None, None, node_width))
    width = units
    for block in heads:
        for head in block:
            # the head's build creates its Dense weights for these widths (layers/conv/gat_conv.py)
            head.ensure_built([(None, None, width), (None, None, edge_width), (None, None, 2)])
        width = units * attention_heads_num if attention_heads_concat else units
    out_mlp.ensure_built((None, width) if output_embedding == "graph" else (None, None, width))
    flat_heads = [head for block in heads for head in block]
    model = _GatModel(name, forward, [embed_n, embed_e, dense0] + flat_heads + [out_mlp],
                      config={"depth": depth, "attention_args": attention_args,
                              "attention_heads_num": attention_heads_num})
    model.__kgcnn_model_version__ = __model_version__
    model.attention_heads = flat_heads
    model.attention_blocks = blocks
    model.fused_attention_blocks = [bool(fused.supported(edge_width)) for fused in blocks]
    model.auto_graph = True   # re-bound inputs replay the whole call sequence from one HIP graph (model/utils.py)
    return model

