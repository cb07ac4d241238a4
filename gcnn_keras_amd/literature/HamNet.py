"""HamNet model builder (mirror of kgcnn/literature/HamNet.py:29-173, ``make_model``; Li, Yang, Song, Cai,
arXiv:2105.03688) on the engine's layers (layers/conv/hamnet_conv.py).

Node and edge attributes go through a tanh Dense, then ``depth`` rounds of ``HamNaiveDynMessage`` (attention whose logit
reads the coordinate differences and the edge row, plus an edge update) and the chosen unions, then either the
fingerprint generator and an MLP, or a per-node MLP.  As in the reference only given coordinates are built: ``q`` is the
coordinate input, ``p = 0``.  Where the sizes fit (``model.fused_hamnet_blocks``: one entry per message step, then the
fingerprint generator) the steps run on csrc/mp_hamnet.hip; every other configuration, every call on a tape (training)
and ``model.use_fused_hamnet = False`` take the layer sequence, one engine call per Keras layer.  The last round's edge
update is read by nobody (the outputs are built from the nodes), so that round's message layer is told not to form it."""
from math import inf

from ..layers.casting import ChangeTensorType
from ..layers.conv.hamnet_conv import HamNaiveDynMessage, HamNetFingerprintGenerator, HamNetGRUUnion, HamNetNaiveUnion
from ..layers.mlp import MLP, GraphMLP
from ..layers.modules import Dense, OptionalInputEmbedding, ZerosLike
from ..model.utils import RouteSwitchModel, update_model_kwargs

__model_version__ = "2022.11.25"

hyper_model_default = {
    "name": "HamNet",
    "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None,), "name": "edge_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": (None, 3), "name": "node_coordinates", "dtype": "float32", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64},
                        "edge": {"input_dim": 5, "output_dim": 64}},
    "message_kwargs": {"units": 128, "units_edge": 128},
    "fingerprint_kwargs": {"units": 128, "units_attend": 128, "depth": 2},
    "gru_kwargs": {"units": 128},
    "verbose": 10, "depth": 1,
    "union_type_node": "gru",
    "union_type_edge": "None",
    "given_coordinates": True,
    "output_embedding": "graph", "output_to_tensor": True,
    "output_mlp": {"use_bias": [True, True, False], "units": [25, 10, 1],
                   "activation": ["relu", "relu", "linear"]}
}


class _HamNetModel(RouteSwitchModel):
    """``Model`` with the ``use_fused_hamnet`` switch over the message steps and the fingerprint generator."""

    switch_attr, switch_layers_attr = "use_fused_hamnet", "hamnet_layers"
    hamnet_layers = ()
    use_fused_hamnet = RouteSwitchModel.switch


def _feature_width(spec, embedding):
    return embedding["output_dim"] if len(spec["shape"]) < 2 else spec["shape"][-1]


def _union(kind, gru_kwargs):
    """HamNet.py:139-152: ``"gru"``, ``"naive"``, anything else takes the update as it is."""
    if kind == "gru":
        return HamNetGRUUnion(**gru_kwargs)
    if kind == "naive":
        return HamNetNaiveUnion(units=gru_kwargs["units"])
    return None


@update_model_kwargs(hyper_model_default, update_recursive=inf)
def make_model(name: str = None, inputs: list = None, input_embedding: dict = None, verbose: int = None,
               message_kwargs: dict = None, gru_kwargs: dict = None, fingerprint_kwargs: dict = None,
               union_type_node: str = None, union_type_edge: str = None, given_coordinates: bool = None,
               depth: int = None, output_embedding: str = None, output_to_tensor: bool = None, output_mlp: dict = None):
    r"""Build HamNet (kgcnn/literature/HamNet.py:107-173).  Model inputs ``[node_attributes, edge_attributes,
    edge_indices, node_coordinates]``, attributes either ``(batch, None, F)`` features or ``(batch, None)`` numbers for an
    embedding.  ``union_type_node`` / ``union_type_edge``: ``"gru"``, ``"naive"`` or ``"None"``.
    ``model.hamnet_layers[i].use_fused_hamnet`` / ``model.use_fused_hamnet`` switch the route."""
    if not given_coordinates:
        raise NotImplementedError("Hamiltonian engine not yet implemented")
    if output_embedding not in ("graph", "node"):
        raise ValueError("Unsupported output embedding for `HamNet`")
    units = gru_kwargs["units"]
    embed_n = OptionalInputEmbedding(**input_embedding["node"], use_embedding=len(inputs[0]["shape"]) < 2)
    embed_e = OptionalInputEmbedding(**input_embedding["edge"], use_embedding=len(inputs[1]["shape"]) < 2)
    zeros = ZerosLike()
    dense_n = Dense(units=units, activation="tanh")
    dense_e = Dense(units=units, activation="tanh")
    messages = [HamNaiveDynMessage(**message_kwargs) for _ in range(depth)]
    node_unions = [_union(union_type_node, gru_kwargs) for _ in messages]
    edge_unions = [_union(union_type_edge, gru_kwargs) for _ in messages]
    if messages:
        messages[-1].return_edge_update = False   # the outputs below read the nodes only
    fingerprint = HamNetFingerprintGenerator(**fingerprint_kwargs) if output_embedding == "graph" else None
    out_mlp = MLP(**output_mlp) if output_embedding == "graph" else GraphMLP(**output_mlp)
    cast = ChangeTensorType(input_tensor_type="ragged", output_tensor_type="tensor") \
        if (output_embedding == "node" and output_to_tensor) else None

    def forward(model_inputs, **kwargs):
        node_input, edge_input, edi, q = model_inputs
        n = dense_n(embed_n(node_input))
        ed = dense_e(embed_e(edge_input))
        p = zeros(q)
        for message, node_union, edge_union in zip(messages, node_unions, edge_unions):
            nu, eu = message([n, ed, p, q, edi], **kwargs)
            n = node_union([n, nu]) if node_union is not None else nu
            if eu is not None:
                ed = edge_union([ed, eu]) if edge_union is not None else eu
        if fingerprint is not None:
            return out_mlp(fingerprint(n, **kwargs))
        out = out_mlp(n)
        return cast(out) if cast is not None else out

    node_width = _feature_width(inputs[0], input_embedding["node"])
    edge_width = _feature_width(inputs[1], input_embedding["edge"])
    coord_width = inputs[3]["shape"][-1]
    embed_n.ensure_built((None, None))
    embed_e.ensure_built((None, None))
    dense_n.ensure_built((None, None, node_width))
    dense_e.ensure_built((None, None, edge_width))
    layers = [embed_n, embed_e, dense_n, dense_e]
    widths = []                                   # (node, edge) width in front of every message step
    nw = ew = units
    for message, node_union, edge_union in zip(messages, node_unions, edge_unions):
        widths.append((nw, ew))
        message.ensure_built([(None, None, nw), (None, None, ew), (None, None, coord_width), (None, None, coord_width),
                              (None, None, 2)])
        layers.append(message)
        if node_union is not None:
            node_union.ensure_built([(None, None, nw), (None, None, message.units)])
            layers.append(node_union)
            nw = units
        else:
            nw = message.units
        if edge_union is not None:
            edge_union.ensure_built([(None, None, ew), (None, None, message.units_edge)])
            layers.append(edge_union)
            ew = units
        else:
            ew = message.units_edge
    if fingerprint is not None:
        fingerprint.ensure_built((None, None, nw))
        layers.append(fingerprint)
    out_mlp.ensure_built((None, fingerprint.units) if fingerprint is not None else (None, None, nw))
    layers.append(out_mlp)
    model = _HamNetModel(name, forward, layers,
                         config={"depth": depth, "message_kwargs": message_kwargs, "gru_kwargs": gru_kwargs,
                                 "fingerprint_kwargs": fingerprint_kwargs, "union_type_node": union_type_node,
                                 "union_type_edge": union_type_edge, "output_embedding": output_embedding})
    model.__kgcnn_model_version__ = __model_version__
    model.message_layers = messages
    model.fingerprint = fingerprint
    model.hamnet_layers = messages + ([fingerprint] if fingerprint is not None else [])
    model.fused_hamnet_blocks = [bool(m.fused_supported(w[0], w[1], coord_width)) for m, w in zip(messages, widths)] + \
        ([bool(fingerprint.fused_supported(nw))] if fingerprint is not None else [])
    model.auto_graph = True   # re-bound inputs replay the whole call sequence from one HIP graph (model/utils.py)
    return model
