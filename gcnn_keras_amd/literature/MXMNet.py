"""MXMNet model builder (mirror of kgcnn/literature/MXMNet.py:24-195): Zhang, Liu, Xie, "Molecular Mechanics-Driven
Graph Neural Network with Multiplex Graph for Molecular Structures" (https://arxiv.org/abs/2011.07457).

Two graphs over one molecule: the *local* bond graph (``edge_indices``) with two angle lists that refer to its edges -
``angle_indices_1`` pairs ``(ij, jk)`` as kgcnn.graph.adj.get_angle_indices gives them with ``edge_pairing="jk"``,
``angle_indices_2`` pairs ``(ij, ik)`` with ``allow_self_edges=True`` - and the *global* range graph
(``range_indices``).  Every block is one ``MXMGlobalMP`` over the range graph and one ``MXMLocalMP`` over the bond graph
(layers/conv/mxmnet_conv.py); the geometry, both bases, the embeddings and the readout are the existing engine layers.

The weights are frozen (``MXMGlobalMP.weight_gradients = False``): inference and forces inside ``EnergyForceModel`` run,
``compile`` + ``train_on_batch`` raises ``NotImplementedError`` and leaves every weight without ``requires_grad``.
"""
from ..layers.casting import ChangeTensorType
from ..layers.conv.dimenet_conv import EmbeddingDimeBlock, SphericalBasisLayer
from ..layers.conv.mxmnet_conv import MXMGlobalMP, MXMLocalMP
from ..layers.geom import BesselBasisLayer, EdgeAngle, NodeDistanceEuclidean, NodePosition
from ..layers.mlp import MLP, GraphMLP
from ..layers.modules import LazyAdd, LazyConcatenate, LazySubtract, OptionalInputEmbedding
from ..layers.pooling import PoolingNodes
from ..model.utils import Model, update_model_kwargs

__model_version__ = "2022.11.25"

model_default = {
    "name": "MXMNet",
    "inputs": [{"shape": (None, ), "name": "node_number", "dtype": "float32", "ragged": True},
               {"shape": (None, 3), "name": "node_coordinates", "dtype": "float32", "ragged": True},
               {"shape": (None, ), "name": "edge_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": [None, 2], "name": "angle_indices_1", "dtype": "int64", "ragged": True},
               {"shape": [None, 2], "name": "angle_indices_2", "dtype": "int64", "ragged": True},
               {"shape": (None, 2), "name": "range_indices", "dtype": "int64", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 32,
                                 "embeddings_initializer": {
                                     "class_name": "RandomUniform",
                                     "config": {"minval": -1.7320508075688772, "maxval": 1.7320508075688772}}},
                        "edge": {"input_dim": 32, "output_dim": 32}},
    "bessel_basis_local": {"num_radial": 16, "cutoff": 5.0, "envelope_exponent": 5},
    "bessel_basis_global": {"num_radial": 16, "cutoff": 5.0, "envelope_exponent": 5},  # Should match range_indices
    "spherical_basis_local": {"num_spherical": 7, "num_radial": 6, "cutoff": 5.0, "envelope_exponent": 5},
    "mlp_rbf_kwargs": {"units": 32, "activation": "swish"},
    "mlp_sbf_kwargs": {"units": 32, "activation": "swish"},
    "global_mp_kwargs": {"units": 32},
    "local_mp_kwargs": {"units": 32, "output_units": 1, "output_kernel_initializer": "zeros"},
    "use_edge_attributes": False,
    "depth": 3,
    "verbose": 10,
    "node_pooling_args": {"pooling_method": "sum"},
    "output_embedding": "graph", "output_to_tensor": True,
    "use_output_mlp": True,
    "output_mlp": {"use_bias": [True], "units": [1],
                   "activation": ["linear"]}
}


class _MxmModel(Model):
    """``Model`` with the ``use_fused_step`` switch over the blocks' three route flags (``MXMGlobalMP.use_fused_step``,
    ``MXMLocalMP.use_fused_step`` and ``.use_fused_triplet``).  Reading it tells whether ALL of them are on; a fresh
    model ships a mix (the global message and the triplet pools fused, the local per-edge messages not),
    so it reads False.  ``True`` switches every fused step on, ``False`` every one off, ``None`` puts back the mix the
    model was built with (``shipped_routes``).  Every change drops the captured HIP graphs, which hold the route they
    were captured on."""

    global_blocks = local_blocks = ()
    _shipped = None

    def _switches(self):
        return tuple(g.use_fused_step for g in self.global_blocks) + \
            tuple(flag for b in self.local_blocks for flag in (b.use_fused_step, b.use_fused_triplet))

    def _set_switches(self, flags):
        flags = tuple(bool(f) for f in flags)
        if flags != self._switches():
            self.release_graphs()
        it = iter(flags)
        for g in self.global_blocks:
            g.use_fused_step = next(it)
        for b in self.local_blocks:
            b.use_fused_step, b.use_fused_triplet = next(it), next(it)

    @property
    def shipped_routes(self):
        """True while every route flag stands as the model was built."""
        return self._switches() == self._shipped

    @property
    def use_fused_step(self):
        return all(self._switches())

    @use_fused_step.setter
    def use_fused_step(self, value):
        if value is None:
            self._set_switches(self._shipped)
        else:
            self._set_switches([bool(value)] * len(self._switches()))

    def _graph_key(self, inputs):
        # the route is part of the identity of a captured graph (a per-layer switch flipped behind the model's back)
        key = Model._graph_key(inputs)
        return None if key is None else key + (self._switches(),)


def _last_units(mlp_kwargs):
    units = mlp_kwargs["units"]
    return int(units[-1] if isinstance(units, (list, tuple)) else units)


@update_model_kwargs(model_default)
def make_model(inputs: list = None, input_embedding: dict = None, depth: int = None, name: str = None,
               bessel_basis_local: dict = None, bessel_basis_global: dict = None, spherical_basis_local: dict = None,
               use_edge_attributes: bool = None, mlp_rbf_kwargs: dict = None, mlp_sbf_kwargs: dict = None,
               global_mp_kwargs: dict = None, local_mp_kwargs: dict = None, verbose: int = None,
               output_embedding: str = None, use_output_mlp: bool = None, node_pooling_args: dict = None,
               output_to_tensor: bool = None, output_mlp: dict = None):
    r"""Build MXMNet (kgcnn/literature/MXMNet.py:56-195).  Model inputs ``[node_attributes, node_coordinates,
    edge_attributes, edge_indices (.., 2), angle_indices_1 (.., 2), angle_indices_2 (.., 2), range_indices (.., 2)]``;
    output ``(batch, L)`` graph embeddings for ``output_embedding="graph"``.  ``output_embedding="node"`` returns, as
    the reference does, the (embedded) input nodes through the output MLP: the message passing does not reach it."""
    if output_embedding not in ("graph", "node"):
        raise ValueError("Unsupported output embedding for mode `MXMNet`")
    use_embedding = len(inputs[0]["shape"]) < 2
    emb = EmbeddingDimeBlock(**input_embedding["node"]) if use_embedding else None
    node_width = int(input_embedding["node"]["output_dim"] if use_embedding else inputs[0]["shape"][-1])
    config = {"inputs": inputs, "input_embedding": input_embedding, "depth": depth,
              "bessel_basis_local": bessel_basis_local, "bessel_basis_global": bessel_basis_global,
              "spherical_basis_local": spherical_basis_local, "use_edge_attributes": use_edge_attributes,
              "mlp_rbf_kwargs": mlp_rbf_kwargs, "mlp_sbf_kwargs": mlp_sbf_kwargs, "global_mp_kwargs": global_mp_kwargs,
              "local_mp_kwargs": local_mp_kwargs, "output_embedding": output_embedding,
              "use_output_mlp": use_output_mlp, "node_pooling_args": node_pooling_args,
              "output_to_tensor": output_to_tensor, "output_mlp": output_mlp}

    if output_embedding == "node":
        # kgcnn/literature/MXMNet.py:178-183: `out = n`.  Keras prunes what the output does not depend on, so the model
        # is the embedding, the output MLP and the cast.
        out_mlp = GraphMLP(**output_mlp) if use_output_mlp else None
        cast = ChangeTensorType(input_tensor_type="ragged", output_tensor_type="tensor") if output_to_tensor else None
        if out_mlp is not None:
            out_mlp.ensure_built((None, None, node_width))

        def forward_node(model_inputs, **kwargs):
            n = emb(model_inputs[0]) if use_embedding else model_inputs[0]
            out = out_mlp(n, **kwargs) if out_mlp is not None else n
            return cast(out) if cast is not None else out

        model = Model(name, forward_node, [x for x in (emb, out_mlp, cast) if x is not None], config=config)
        model.__kgcnn_model_version__ = __model_version__
        model.fused = None
        model.auto_graph = True
        return model

    embed_e = OptionalInputEmbedding(**input_embedding["edge"], use_embedding=len(inputs[2]["shape"]) < 2)
    pos_l, dist_l = NodePosition(), NodeDistanceEuclidean()
    bessel_l = BesselBasisLayer(**bessel_basis_local)
    subtract = LazySubtract()
    angle_1 = EdgeAngle()
    angle_2 = EdgeAngle(vector_scale=[1.0, -1.0])
    sbf_1 = SphericalBasisLayer(**spherical_basis_local)
    sbf_2 = SphericalBasisLayer(**spherical_basis_local)
    pos_g, dist_g = NodePosition(), NodeDistanceEuclidean()
    bessel_g = BesselBasisLayer(**bessel_basis_global)
    cat_e = LazyConcatenate() if use_edge_attributes else None
    mlp_rbf_l = GraphMLP(**mlp_rbf_kwargs)
    mlp_sbf_1 = GraphMLP(**mlp_sbf_kwargs)
    mlp_sbf_2 = GraphMLP(**mlp_sbf_kwargs)
    mlp_rbf_g = GraphMLP(**mlp_rbf_kwargs)
    globals_, locals_ = [], []
    for _ in range(depth):
        globals_.append(MXMGlobalMP(**global_mp_kwargs))
        locals_.append(MXMLocalMP(**local_mp_kwargs))
    add_out = LazyAdd()
    pool = PoolingNodes(**node_pooling_args)
    out_mlp = MLP(**output_mlp) if use_output_mlp else None

    def forward(model_inputs, **kwargs):
        node_input, x, edge_input, ei_l, ai_1, ai_2, ri_g = model_inputs
        n = emb(node_input) if use_embedding else node_input

        # distances, Bessel and spherical bases of the local edges and their two angle lists
        pos1_l, pos2_l = pos_l([x, ei_l])
        d_l = dist_l([pos1_l, pos2_l])
        rbf_l = bessel_l(d_l)
        v12_l = subtract([pos1_l, pos2_l])
        a_l_1 = angle_1([v12_l, ai_1])
        a_l_2 = angle_2([v12_l, ai_2])
        sbf_l_1 = sbf_1([d_l, a_l_1, ai_1])
        sbf_l_2 = sbf_2([d_l, a_l_2, ai_2])

        # distance and Bessel basis of the global (range) edges
        pos1_g, pos2_g = pos_g([x, ri_g])
        d_g = dist_g([pos1_g, pos2_g])
        rbf_g = bessel_g(d_g)

        if use_edge_attributes:
            rbf_l = cat_e([rbf_l, embed_e(edge_input)])

        rbf_l = mlp_rbf_l(rbf_l)
        sbf_l_1 = mlp_sbf_1(sbf_l_1)
        sbf_l_2 = mlp_sbf_2(sbf_l_2)
        rbf_g = mlp_rbf_g(rbf_g)

        h = n
        nodes_list = []
        for glob, loc in zip(globals_, locals_):
            h = glob([h, rbf_g, ri_g])
            h, t = loc([h, rbf_l, sbf_l_1, sbf_l_2, ei_l, ai_1, ai_2])
            nodes_list.append(t)

        out = add_out(nodes_list)
        out = pool(out)
        return out_mlp(out) if out_mlp is not None else out

    # weights exist before the first call (set_weights / get_weights)
    num_radial_l = int(bessel_basis_local["num_radial"])
    if use_edge_attributes:
        embed_e.ensure_built((None,) + tuple(inputs[2]["shape"]))
        num_radial_l += int(input_embedding["edge"]["output_dim"] if embed_e.use_embedding else inputs[2]["shape"][-1])
    nsbf = int(spherical_basis_local["num_spherical"]) * int(spherical_basis_local["num_radial"])
    mlp_rbf_l.ensure_built((None, None, num_radial_l))
    mlp_sbf_1.ensure_built((None, None, nsbf))
    mlp_sbf_2.ensure_built((None, None, nsbf))
    mlp_rbf_g.ensure_built((None, None, int(bessel_basis_global["num_radial"])))
    rbf_w, sbf_w = _last_units(mlp_rbf_kwargs), _last_units(mlp_sbf_kwargs)
    width = node_width
    pair = (None, None, 2)
    for glob, loc in zip(globals_, locals_):
        glob.ensure_built([(None, None, width), (None, None, rbf_w), pair])
        width = glob.dim
        loc.ensure_built([(None, None, width), (None, None, rbf_w), (None, None, sbf_w), (None, None, sbf_w), pair,
                          pair, pair])
        width = loc.dim
    if out_mlp is not None:
        out_mlp.ensure_built((None, locals_[-1].output_dim if locals_ else node_width))

    layers = [x for x in (emb, embed_e if use_edge_attributes else None, pos_l, dist_l, bessel_l, subtract, angle_1,
                          angle_2, sbf_1, sbf_2, pos_g, dist_g, bessel_g, cat_e, mlp_rbf_l, mlp_sbf_1, mlp_sbf_2,
                          mlp_rbf_g) if x is not None]
    for glob, loc in zip(globals_, locals_):
        layers += [glob, loc]
    layers += [add_out, pool] + ([out_mlp] if out_mlp is not None else [])
    model = _MxmModel(name, forward, layers, config=config)
    model.__kgcnn_model_version__ = __model_version__
    model.fused = None
    model.global_blocks, model.local_blocks = globals_, locals_
    model._shipped = model._switches()
    # the layer sequence is replayed from one HIP graph for re-bound inputs (model/utils.py)
    model.auto_graph = True
    return model
