"""RGCN model builder (mirror of kgcnn/literature/RGCN.py:23-119, ``make_model``): relational graph convolution
(Schlichtkrull et al. 2017, https://arxiv.org/abs/1703.06103).

Each of ``depth`` blocks is one ``RGCNStep`` (``layers/conv/rgcn_conv.py``): every edge sends its sender's features through
the kernel of the edge's relation, scaled by the edge weight; the receiver sums them, adds its own ``Dense`` and applies the
activation.  Blocks whose sizes fit run on the fused kernel of csrc/mp_rgcn.hip outside a tape, one launch per block;
``model.fused_relational_blocks`` lists which do, ``model.use_fused_relational`` (or ``block.use_fused_relational``)
switches the route.  Training (``compile`` / ``train_on_batch``) goes through the layer sequence.  ``num_bases`` /
``num_blocks`` in ``dense_relation_kwargs`` select the paper's two kernel decompositions.
"""
from ..layers.casting import ChangeTensorType
from ..layers.conv.rgcn_conv import RGCNStep
from ..layers.mlp import MLP, GraphMLP
from ..layers.modules import OptionalInputEmbedding
from ..layers.pooling import PoolingNodes
from ..model.utils import RouteSwitchModel, update_model_kwargs

__model_version__ = "2022.11.25"

model_default = {
    "name": "RGCN",
    "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": (None, 1), "name": "edge_weights", "dtype": "float32", "ragged": True},
               {"shape": (None,), "name": "edge_relations", "dtype": "int64", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64}},
    "dense_relation_kwargs": {"units": 64, "num_relations": 20},
    "dense_kwargs": {"units": 64},
    "activation_kwargs": {"activation": "swish"},
    "depth": 3, "verbose": 10,
    "output_embedding": "graph", "output_to_tensor": True,
    "output_mlp": {"use_bias": True, "units": 1,
                   "activation": "softmax"}
}


class _RelationalModel(RouteSwitchModel):
    """``Model`` with the ``use_fused_relational`` switch over all blocks (shared with ``GNNFilm``)."""

    switch_attr, switch_layers_attr = "use_fused_relational", "relational_layers"
    relational_layers = ()
    use_fused_relational = RouteSwitchModel.switch


def _width(spec, embedding):
    return embedding["output_dim"] if len(spec["shape"]) < 2 else spec["shape"][-1]


@update_model_kwargs(model_default)
def make_model(inputs: list = None, input_embedding: dict = None, depth: int = None,
               dense_relation_kwargs: dict = None, dense_kwargs: dict = None, activation_kwargs: dict = None,
               name: str = None, verbose: int = None, output_embedding: str = None, output_to_tensor: bool = None,
               output_mlp: dict = None):
    r"""Build RGCN (kgcnn/literature/RGCN.py:85-119).  Model inputs ``[node_attributes, edge_indices, edge_weights,
    edge_relations]``: nodes as integer types ``(batch, [N])`` for the embedding or as features ``(batch, [N], F)``, edge
    weights ``(batch, [M], 1)``, relations ``(batch, [M])`` int64.  Output: ``(batch, L)`` for
    ``output_embedding="graph"``, per node for ``"node"``."""
    if output_embedding not in ("graph", "node"):
        raise ValueError("Unsupported output embedding for mode `RGCN`")
    embed_n = OptionalInputEmbedding(**input_embedding["node"], use_embedding=len(inputs[0]["shape"]) < 2)
    # new layers in every block (the reference creates them inside its loop)
    blocks = [RGCNStep(dense_kwargs=dense_kwargs, dense_relation_kwargs=dense_relation_kwargs,
                       activation_kwargs=activation_kwargs) for _ in range(depth)]
    pool = PoolingNodes() if output_embedding == "graph" else None
    out_mlp = MLP(**output_mlp) if output_embedding == "graph" else GraphMLP(**output_mlp)
    cast = ChangeTensorType(input_tensor_type="ragged", output_tensor_type="tensor") \
        if (output_embedding == "node" and output_to_tensor) else None

    def forward(model_inputs, **kwargs):
        node_input, edi, edge_weights, edge_relations = model_inputs
        n = embed_n(node_input)
        for block in blocks:
            n = block([n, edi, edge_weights, edge_relations], **kwargs)
        if output_embedding == "graph":
            return out_mlp(pool(n))
        out = out_mlp(n)
        return cast(out) if cast is not None else out

    width = _width(inputs[0], input_embedding["node"])
    weight_shape = (None,) + tuple(inputs[2]["shape"])
    embed_n.ensure_built((None, None))
    for block in blocks:
        block.ensure_built([(None, None, width), (None, None, 2), weight_shape, (None, None)])
        width = block.units
    out_mlp.ensure_built((None, width) if output_embedding == "graph" else (None, None, width))
    model = _RelationalModel(name, forward, [embed_n] + blocks + [out_mlp],
                             config={"depth": depth, "dense_relation_kwargs": dense_relation_kwargs,
                                     "dense_kwargs": dense_kwargs, "activation_kwargs": activation_kwargs})
    model.__kgcnn_model_version__ = __model_version__
    model.relational_layers = blocks
    model.fused_relational_blocks = [bool(block.fused_relational) for block in blocks]
    # re-bound inputs replay the whole forward from one HIP graph (model/utils.py); the route is part of its identity
    model.auto_graph = True
    return model
