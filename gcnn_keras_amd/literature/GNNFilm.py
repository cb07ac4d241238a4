"""GNNFilm model builder (mirror of kgcnn/literature/GNNFilm.py:23-117, ``make_model``): graph network with feature-wise
linear modulation (Brockschmidt 2019, https://arxiv.org/abs/1906.12192).

Each of ``depth`` blocks is one ``GNNFilmStep`` (``layers/conv/rgcn_conv.py``): every edge sends its sender's features
through the kernel of the edge's relation; the receiver scales the message by ``gamma`` and shifts it by ``beta``, two
relational functions of its OWN features, sums and applies the activation.  Blocks whose sizes fit run on the fused kernel
of csrc/mp_rgcn.hip outside a tape, one launch per block instead of three edge-sized ``RelationalDense`` calls;
``model.fused_relational_blocks`` lists which do, ``model.use_fused_relational`` (or ``block.use_fused_relational``)
switches the route.  Training (``compile`` / ``train_on_batch``) goes through the layer sequence.
"""
from ..layers.casting import ChangeTensorType
from ..layers.conv.rgcn_conv import GNNFilmStep
from ..layers.mlp import MLP, GraphMLP
from ..layers.modules import OptionalInputEmbedding
from ..layers.pooling import PoolingNodes
from ..model.utils import update_model_kwargs
from .RGCN import _RelationalModel, _width

__model_version__ = "2022.11.25"

model_default = {
    "name": "GNNFilm",
    "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": (None,), "name": "edge_relations", "dtype": "int64", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64}},
    "dense_relation_kwargs": {"units": 64, "num_relations": 20},
    "dense_modulation_kwargs": {"units": 64, "num_relations": 20, "activation": "sigmoid"},
    "activation_kwargs": {"activation": "swish"},
    "depth": 3, "verbose": 10,
    "output_embedding": "graph", "output_to_tensor": True,
    "output_mlp": {"use_bias": True, "units": 1,
                   "activation": "softmax"}
}


@update_model_kwargs(model_default)
def make_model(inputs: list = None, input_embedding: dict = None, depth: int = None,
               dense_relation_kwargs: dict = None, dense_modulation_kwargs: dict = None,
               activation_kwargs: dict = None, name: str = None, verbose: int = None, output_embedding: str = None,
               output_to_tensor: bool = None, output_mlp: dict = None):
    r"""Build GNNFilm (kgcnn/literature/GNNFilm.py:83-117).  Model inputs ``[node_attributes, edge_indices,
    edge_relations]``: nodes as integer types ``(batch, [N])`` for the embedding or as features ``(batch, [N], F)``,
    relations ``(batch, [M])`` int64.  Output: ``(batch, L)`` for ``output_embedding="graph"``, per node for ``"node"``."""
    if output_embedding not in ("graph", "node"):
        raise ValueError("Unsupported output embedding for mode `GNNFilm`")
    embed_n = OptionalInputEmbedding(**input_embedding["node"], use_embedding=len(inputs[0]["shape"]) < 2)
    # new layers in every block (the reference creates them inside its loop)
    blocks = [GNNFilmStep(dense_relation_kwargs=dense_relation_kwargs, dense_modulation_kwargs=dense_modulation_kwargs,
                          activation_kwargs=activation_kwargs) for _ in range(depth)]
    pool = PoolingNodes() if output_embedding == "graph" else None
    out_mlp = MLP(**output_mlp) if output_embedding == "graph" else GraphMLP(**output_mlp)
    cast = ChangeTensorType(input_tensor_type="ragged", output_tensor_type="tensor") \
        if (output_embedding == "node" and output_to_tensor) else None

    def forward(model_inputs, **kwargs):
        node_input, edi, edge_relations = model_inputs
        n = embed_n(node_input)
        for block in blocks:
            n = block([n, edi, edge_relations], **kwargs)
        if output_embedding == "graph":
            return out_mlp(pool(n))
        out = out_mlp(n)
        return cast(out) if cast is not None else out

    width = _width(inputs[0], input_embedding["node"])
    embed_n.ensure_built((None, None))
    for block in blocks:
        block.ensure_built([(None, None, width), (None, None, 2), (None, None)])
        width = block.units
    out_mlp.ensure_built((None, width) if output_embedding == "graph" else (None, None, width))
    model = _RelationalModel(name, forward, [embed_n] + blocks + [out_mlp],
                             config={"depth": depth, "dense_relation_kwargs": dense_relation_kwargs,
                                     "dense_modulation_kwargs": dense_modulation_kwargs,
                                     "activation_kwargs": activation_kwargs})
    model.__kgcnn_model_version__ = __model_version__
    model.relational_layers = blocks
    model.fused_relational_blocks = [bool(block.fused_relational) for block in blocks]
    # re-bound inputs replay the whole forward from one HIP graph (model/utils.py); the route is part of its identity
    model.auto_graph = True
    return model
