"""AttentiveFP model builder (mirror of kgcnn/literature/AttentiveFP.py:25-127, ``make_model``; Xiong et al., J. Med. Chem.
2020, 63, 16, 8749-8760) on the engine's layers (layers/conv/attentivefp_conv.py).

``depthato`` rounds of attention head + ``GRUUpdate`` on the atoms (the first head reads the edge features), then either
the attentive readout (``depthmol`` iterations) and an MLP, or a per-node MLP.  Where the sizes fit
(``model.fused_attentive_blocks``: one entry per head, then the readout) the heads and the readout run on
csrc/mp_attentivefp.hip and csrc/mp_gat.hip; every other configuration, every call on a tape (training) and
``model.use_fused_attentive = False`` take the layer sequence, one engine call per Keras layer.  ``Dropout`` is the
inference identity."""
from ..layers.casting import ChangeTensorType
from ..layers.conv.attentivefp_conv import AttentiveHeadFP, PoolingNodesAttentive
from ..layers.conv.mpnn_conv import GRUUpdate
from ..layers.mlp import MLP, GraphMLP
from ..layers.modules import Dense, Dropout, OptionalInputEmbedding
from ..model.utils import RouteSwitchModel, update_model_kwargs

__model_version__ = "2022.11.25"

model_default = {
    "name": "AttentiveFP",
    "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None,), "name": "edge_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64},
                        "edge": {"input_dim": 5, "output_dim": 64}},
    "attention_args": {"units": 32},
    "depthmol": 2,
    "depthato": 2,
    "dropout": 0.1,
    "verbose": 10,
    "output_embedding": "graph", "output_to_tensor": True,
    "output_mlp": {"use_bias": [True, True, False], "units": [25, 10, 1],
                   "activation": ["relu", "relu", "sigmoid"]}
}


class _AttentiveFPModel(RouteSwitchModel):
    """``Model`` with the ``use_fused_attentive`` switch over the heads and the readout."""

    switch_attr, switch_layers_attr = "use_fused_attentive", "attentive_layers"
    attentive_layers = ()
    use_fused_attentive = RouteSwitchModel.switch


def _feature_width(spec, embedding):
    return embedding["output_dim"] if len(spec["shape"]) < 2 else spec["shape"][-1]


@update_model_kwargs(model_default)
def make_model(inputs: list = None, input_embedding: dict = None, depthmol: int = None, depthato: int = None,
               dropout: float = None, attention_args: dict = None, name: str = None, verbose: int = None,
               output_embedding: str = None, output_to_tensor: bool = None, output_mlp: dict = None):
    r"""Build AttentiveFP (kgcnn/literature/AttentiveFP.py:90-127).  Model inputs ``[node_attributes, edge_attributes,
    edge_indices]``, attributes either ``(batch, None, F)`` features or ``(batch, None)`` numbers for an embedding.
    ``attention_args`` go to every ``AttentiveHeadFP``; its ``units`` are also the ``GRUUpdate`` and readout width.
    ``model.attentive_layers[i].use_fused_attentive`` / ``model.use_fused_attentive`` switch the route."""
    if output_embedding not in ("graph", "node"):
        raise ValueError("Unsupported graph embedding for mode `AttentiveFP`")
    units = attention_args["units"]
    embed_n = OptionalInputEmbedding(**input_embedding["node"], use_embedding=len(inputs[0]["shape"]) < 2)
    embed_e = OptionalInputEmbedding(**input_embedding["edge"], use_embedding=len(inputs[1]["shape"]) < 2)
    dense0 = Dense(units=units)
    heads = [AttentiveHeadFP(use_edge_features=(i == 0), **attention_args) for i in range(max(depthato, 1))]
    updates = [GRUUpdate(units=units) for _ in heads]
    drops = [None] + [Dropout(rate=dropout) for _ in heads[1:]]
    readout = PoolingNodesAttentive(units=units, depth=depthmol) if output_embedding == "graph" else None
    out_mlp = MLP(**output_mlp) if output_embedding == "graph" else GraphMLP(**output_mlp)
    cast = ChangeTensorType(input_tensor_type="ragged", output_tensor_type="tensor") \
        if (output_embedding == "node" and output_to_tensor) else None

    def forward(model_inputs, **kwargs):
        node_input, edge_input, edi = model_inputs
        nk = dense0(embed_n(node_input))
        ed = embed_e(edge_input)
        for head, update, drop in zip(heads, updates, drops):
            ck = head([nk, ed, edi], **kwargs)
            nk = update([nk, ck])
            if drop is not None:
                nk = drop(nk, **kwargs)
        if readout is not None:
            return out_mlp(readout(nk, **kwargs))
        out = out_mlp(nk)
        return cast(out) if cast is not None else out

    node_width = _feature_width(inputs[0], input_embedding["node"])
    edge_width = _feature_width(inputs[1], input_embedding["edge"])
    embed_n.ensure_built((None, None))
    embed_e.ensure_built((None, None))
    dense0.ensure_built((None, None, node_width))
    for head, update in zip(heads, updates):
        # the head's build creates its Dense weights for these widths (layers/conv/attentivefp_conv.py)
        head.ensure_built([(None, None, units), (None, None, edge_width), (None, None, 2)])
        update.ensure_built([(None, None, units), (None, None, units)])
    if readout is not None:
        readout.ensure_built((None, None, units))
    out_mlp.ensure_built((None, units) if output_embedding == "graph" else (None, None, units))
    layers = [embed_n, embed_e, dense0]
    for head, update in zip(heads, updates):
        layers += [head, update]
    layers += ([readout] if readout is not None else []) + [out_mlp]
    model = _AttentiveFPModel(name, forward, layers,
                              config={"depthato": depthato, "depthmol": depthmol, "attention_args": attention_args,
                                      "output_embedding": output_embedding})
    model.__kgcnn_model_version__ = __model_version__
    model.attention_heads = heads
    model.readout = readout
    model.attentive_layers = heads + ([readout] if readout is not None else [])
    model.fused_attentive_blocks = [bool(head.fused_supported(edge_width)) for head in heads] + \
        ([bool(readout.fused_supported())] if readout is not None else [])
    model.auto_graph = True   # re-bound inputs replay the whole call sequence from one HIP graph (model/utils.py)
    return model
