"""DimeNet++ model builder (mirror of kgcnn/literature/DimeNetPP.py:23-183): Klicpera et al., "Fast and
Uncertainty-Aware Directional Message Passing for Non-Equilibrium Molecules" (https://arxiv.org/abs/2011.14115).

Edge messages pass from edge to edge over angle pairs ``(n, m)`` = ``((i, j), (j, k))`` (``angle_indices`` refer to
edges, as kgcnn.graph.adj.get_angle_indices with ``edge_pairing="jk"`` gives them).  The spherical basis and the
triplet step of every interaction block run on csrc/mp_dimenet.hip (layers/conv/dimenet_conv.py); everything else on
the existing engine layers.  Only ``output_embedding="graph"`` is built, as in the reference; ``make_crystal_model``
(periodic images) raises ``NotImplementedError``.
"""
from ..layers.conv.dimenet_conv import DimNetInteractionPPBlock, DimNetOutputBlock, EmbeddingDimeBlock, \
    SphericalBasisLayer
from ..layers.gather import GatherNodes
from ..layers.geom import BesselBasisLayer, EdgeAngle, NodeDistanceEuclidean, NodePosition
from ..layers.mlp import MLP
from ..layers.modules import Dense, LazyAdd, LazyConcatenate, LazySubtract
from ..layers.pooling import PoolingNodes
from ..model.utils import Model, update_model_kwargs

__model_version__ = "2022.11.25"

model_default = {
    "name": "DimeNetPP",
    "inputs": [{"shape": [None], "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": [None, 3], "name": "node_coordinates", "dtype": "float32", "ragged": True},
               {"shape": [None, 2], "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": [None, 2], "name": "angle_indices", "dtype": "int64", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 128,
                                 "embeddings_initializer": {"class_name": "RandomUniform",
                                                            "config": {"minval": -1.7320508075688772,
                                                                       "maxval": 1.7320508075688772}}}},
    "emb_size": 128, "out_emb_size": 256, "int_emb_size": 64, "basis_emb_size": 8,
    "num_blocks": 4, "num_spherical": 7, "num_radial": 6,
    "cutoff": 5.0, "envelope_exponent": 5,
    "num_before_skip": 1, "num_after_skip": 2, "num_dense_output": 3,
    "num_targets": 64, "extensive": True, "output_init": "zeros",
    "activation": "swish", "verbose": 10,
    "output_embedding": "graph",
    "use_output_mlp": True,
    "output_mlp": {"use_bias": [True, False],
                   "units": [64, 12], "activation": ["swish", "linear"]}
}


@update_model_kwargs(model_default)
def make_model(inputs: list = None, input_embedding: dict = None, emb_size: int = None, out_emb_size: int = None,
               int_emb_size: int = None, basis_emb_size: int = None, num_blocks: int = None, num_spherical: int = None,
               num_radial: int = None, cutoff: float = None, envelope_exponent: int = None,
               num_before_skip: int = None, num_after_skip: int = None, num_dense_output: int = None,
               num_targets: int = None, activation: str = None, extensive: bool = None, output_init: str = None,
               verbose: int = None, name: str = None, output_embedding: str = None, use_output_mlp: bool = None,
               output_mlp: dict = None):
    r"""Build DimeNet++ (kgcnn/literature/DimeNetPP.py:47-183).  Model inputs ``[node_attributes, node_coordinates,
    edge_indices (.., 2), angle_indices (.., 2)]``; output ``(batch, L)`` graph embeddings."""
    if output_embedding != "graph":
        raise ValueError("Unsupported output embedding for mode `DimeNetPP`.")
    use_embedding = len(inputs[0]["shape"]) == 1
    emb = EmbeddingDimeBlock(**input_embedding["node"]) if use_embedding else None
    node_position = NodePosition()
    distance = NodeDistanceEuclidean()
    bessel = BesselBasisLayer(num_radial=num_radial, cutoff=cutoff, envelope_exponent=envelope_exponent)
    subtract = LazySubtract()
    edge_angle = EdgeAngle()
    sbf_layer = SphericalBasisLayer(num_spherical=num_spherical, num_radial=num_radial, cutoff=cutoff,
                                    envelope_exponent=envelope_exponent)
    rbf_dense = Dense(emb_size, use_bias=True, activation=activation, kernel_initializer="kgcnn>glorot_orthogonal")
    gather_pairs = GatherNodes()
    concat = LazyConcatenate(axis=-1)
    x_dense = Dense(emb_size, use_bias=True, activation=activation, kernel_initializer="kgcnn>glorot_orthogonal")
    out0 = DimNetOutputBlock(emb_size, out_emb_size, num_dense_output, num_targets=num_targets,
                             output_kernel_initializer=output_init)
    blocks, outs = [], []
    for _ in range(num_blocks):
        blocks.append(DimNetInteractionPPBlock(emb_size, int_emb_size, basis_emb_size, num_before_skip,
                                               num_after_skip))
        outs.append(DimNetOutputBlock(emb_size, out_emb_size, num_dense_output, num_targets=num_targets,
                                      output_kernel_initializer=output_init))
    add_xp = LazyAdd()
    pool = PoolingNodes(pooling_method="sum" if extensive else "mean")
    out_mlp = MLP(**output_mlp) if use_output_mlp else None

    def forward(model_inputs, **kwargs):
        node_input, xyz_input, bond_index_input, angle_index_input = model_inputs
        n = emb(node_input) if use_embedding else node_input
        pos1, pos2 = node_position([xyz_input, bond_index_input])
        d = distance([pos1, pos2])
        rbf = bessel(d)
        v12 = subtract([pos1, pos2])
        a = edge_angle([v12, angle_index_input])
        sbf = sbf_layer([d, a, angle_index_input])
        rbf_emb = rbf_dense(rbf)
        n_pairs = gather_pairs([n, bond_index_input])
        x = concat([n_pairs, rbf_emb])
        x = x_dense(x)
        ps = out0([n, x, rbf, bond_index_input])
        for block, out_block in zip(blocks, outs):
            x = block([x, rbf, sbf, angle_index_input])
            ps = add_xp([ps, out_block([n, x, rbf, bond_index_input])])
        out = pool(ps)
        return out_mlp(out) if out_mlp is not None else out

    # weights exist before the first call (set_weights / get_weights)
    node_width = input_embedding["node"]["output_dim"] if use_embedding else inputs[0]["shape"][-1]
    nsbf = num_spherical * num_radial
    rbf_dense.ensure_built((None, None, num_radial))
    x_dense.ensure_built((None, None, 2 * node_width + emb_size))
    edge_shapes = [(None, None, node_width), (None, None, emb_size), (None, None, num_radial), (None, None, 2)]
    for out_block in [out0] + outs:
        out_block.ensure_built(edge_shapes)
    for block in blocks:
        block.ensure_built([(None, None, emb_size), (None, None, num_radial), (None, None, nsbf), (None, None, 2)])
    if out_mlp is not None:
        out_mlp.ensure_built((None, num_targets))
    layers = [x for x in [emb, node_position, distance, bessel, subtract, edge_angle, sbf_layer, rbf_dense,
                          gather_pairs, concat, x_dense, out0] if x is not None]
    for block, out_block in zip(blocks, outs):
        layers += [block, out_block]
    layers += [add_xp, pool] + ([out_mlp] if out_mlp is not None else [])
    config = {"input_embedding": input_embedding, "emb_size": emb_size, "out_emb_size": out_emb_size,
              "int_emb_size": int_emb_size, "basis_emb_size": basis_emb_size, "num_blocks": num_blocks,
              "num_spherical": num_spherical, "num_radial": num_radial, "cutoff": cutoff,
              "envelope_exponent": envelope_exponent, "num_before_skip": num_before_skip,
              "num_after_skip": num_after_skip, "num_dense_output": num_dense_output, "num_targets": num_targets,
              "activation": activation, "extensive": extensive, "output_init": output_init,
              "use_output_mlp": use_output_mlp, "output_mlp": output_mlp}
    model = Model(name, forward, layers, config=config)
    model.__kgcnn_model_version__ = __model_version__
    model.fused = None
    # the layer sequence is replayed from one HIP graph for re-bound inputs (model/utils.py)
    model.auto_graph = True
    return model


def make_crystal_model(**kwargs):
    """The periodic DimeNet++ (kgcnn/literature/DimeNetPP.py:186-339) is not implemented; use ``make_model``."""
    raise NotImplementedError("DimeNetPP.make_crystal_model (periodic images) is not implemented; use make_model")
