"""SchNet model builders (mirror of kgcnn/literature/Schnet.py:24-282, ``make_model`` and ``make_crystal_model``).

``make_model(**kwargs)`` accepts the reference's keyword dictionary (validated against ``model_default`` by
``update_model_kwargs``) and returns a callable model taking ``[node_attributes, node_coordinates, edge_indices]``
as ragged tensors.  Configurations that fit the fused kernels (``gcnn_keras_amd.fused.supports``: the reference's
defaults at any depth) run the whole forward in eight HIP kernels on the model's own weight tensors
(``model.fused``: the route object - launch mode, bound batches); everything else, and any call that asks for
gradients, runs the reference's layer sequence op by op.  Weights are created in constructor order, so ``model.set_weights`` accepts the list that
``gcnn_keras_amd.synth.schnet_params`` / a Keras ``get_weights()`` of the reference model produce.

``make_crystal_model(**kwargs)`` is the periodic variant: inputs ``[node_attributes, node_coordinates, edge_indices,
edge_image, graph_lattice]``, the last a dense ``(batch, 3, 3)`` tensor with the lattice vectors in rows; the sender
position of every edge is shifted by ``edge_image @ lattice`` (``ShiftPeriodicLattice``) before the distance is taken.
Same layers and weight order as ``make_model``.  It always runs the layer path (``model.fused`` is ``None``), replayed
from one HIP graph per bound batch (``auto_graph``).
"""
from ..layers.casting import ChangeTensorType
from ..layers.conv.schnet_conv import SchNetInteraction
from ..layers.geom import GaussBasisLayer, NodeDistanceEuclidean, NodePosition, ShiftPeriodicLattice
from ..layers.mlp import MLP, GraphMLP
from ..layers.modules import Dense, OptionalInputEmbedding
from ..layers.pooling import PoolingNodes
from .. import fused as _fused
from ..model.utils import Model, update_model_kwargs

__model_version__ = "2022.11.25"

model_default = {
    "name": "Schnet",
    "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 3), "name": "node_coordinates", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64}},
    "make_distance": True, "expand_distance": True,
    "interaction_args": {"units": 128, "use_bias": True,
                         "activation": "kgcnn>shifted_softplus", "cfconv_pool": "sum"},
    "node_pooling_args": {"pooling_method": "sum"},
    "depth": 4,
    "gauss_args": {"bins": 20, "distance": 4, "offset": 0.0, "sigma": 0.4},
    "verbose": 10,
    "last_mlp": {"use_bias": [True, True], "units": [128, 64],
                 "activation": ["kgcnn>shifted_softplus", "kgcnn>shifted_softplus"]},
    "output_embedding": "graph", "output_to_tensor": True,
    "use_output_mlp": True,
    "output_mlp": {"use_bias": [True, True], "units": [64, 1],
                   "activation": ["kgcnn>shifted_softplus", "linear"]}
}

model_crystal_default = {
    "name": "Schnet",
    "inputs": [{"shape": (None,), "name": "node_number", "dtype": "float32", "ragged": True},
               {"shape": (None, 3), "name": "node_coordinates", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": (None, 3), "name": "edge_image", "dtype": "int64", "ragged": True},
               {"shape": (3, 3), "name": "graph_lattice", "dtype": "float32", "ragged": False}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64}},
    "make_distance": True, "expand_distance": True,
    "interaction_args": {"units": 128, "use_bias": True, "activation": "kgcnn>shifted_softplus", "cfconv_pool": "sum"},
    "node_pooling_args": {"pooling_method": "sum"},
    "depth": 4,
    "gauss_args": {"bins": 20, "distance": 4, "offset": 0.0, "sigma": 0.4},
    "verbose": 10,
    "last_mlp": {"use_bias": [True, True], "units": [128, 64],
                 "activation": ["kgcnn>shifted_softplus", "kgcnn>shifted_softplus"]},
    "output_embedding": "graph", "output_to_tensor": True,
    "use_output_mlp": True,
    "output_mlp": {"use_bias": [True, True], "units": [64, 1],
                   "activation": ["kgcnn>shifted_softplus", "linear"]}
}


@update_model_kwargs(model_default)
def make_model(inputs: list = None, input_embedding: dict = None, make_distance: bool = None,
               expand_distance: bool = None, gauss_args: dict = None, interaction_args: dict = None,
               node_pooling_args: dict = None, depth: int = None, name: str = None, verbose: int = None,
               last_mlp: dict = None, output_embedding: str = None, use_output_mlp: bool = None,
               output_to_tensor: bool = None, output_mlp: dict = None):
    r"""Build SchNet (kgcnn/literature/Schnet.py:46-148).  Inputs of the returned model:
    ``[node_attributes, edge_distance | node_coordinates, edge_indices]`` ragged; output ``(batch, L)`` tensor for
    ``output_embedding="graph"``."""
    return _make(False, inputs, input_embedding, make_distance, expand_distance, gauss_args, interaction_args,
                 node_pooling_args, depth, name, last_mlp, output_embedding, use_output_mlp, output_to_tensor,
                 output_mlp)


@update_model_kwargs(model_default)   # the reference decorates it with the molecular defaults
def make_crystal_model(inputs: list = None, input_embedding: dict = None, make_distance: bool = None,
                       expand_distance: bool = None, gauss_args: dict = None, interaction_args: dict = None,
                       node_pooling_args: dict = None, depth: int = None, name: str = None, verbose: int = None,
                       last_mlp: dict = None, output_embedding: str = None, use_output_mlp: bool = None,
                       output_to_tensor: bool = None, output_mlp: dict = None):
    r"""Build SchNet for periodic structures (kgcnn/literature/Schnet.py:174-282).  Inputs of the returned model:
    ``[node_attributes, edge_distance | node_coordinates, edge_indices, edge_image, graph_lattice]``; ``edge_image``
    ragged ``(batch, [M], 3)`` int64, ``graph_lattice`` dense ``(batch, 3, 3)``.  As in the reference the keyword defaults
    are those of ``make_model``, so ``inputs`` has to be given: ``model_crystal_default["inputs"]``."""
    if inputs is None or len(inputs) < 5:
        raise ValueError("Schnet.make_crystal_model needs five inputs (node, xyz, edge_indices, edge_image, "
                         "graph_lattice): pass inputs=model_crystal_default[\"inputs\"] (the keyword defaults are those "
                         "of make_model, as in the reference)")
    return _make(True, inputs, input_embedding, make_distance, expand_distance, gauss_args, interaction_args,
                 node_pooling_args, depth, name, last_mlp, output_embedding, use_output_mlp, output_to_tensor,
                 output_mlp)


def _make(crystal, inputs, input_embedding, make_distance, expand_distance, gauss_args, interaction_args,
          node_pooling_args, depth, name, last_mlp, output_embedding, use_output_mlp, output_to_tensor, output_mlp):
    """Both builders: the same layers in the same order; ``crystal`` adds the lattice shift of the sender positions."""
    if output_embedding not in ("graph", "node"):
        raise ValueError("Unsupported output embedding for mode `SchNet`")

    embed = OptionalInputEmbedding(**input_embedding["node"], use_embedding=len(inputs[0]["shape"]) < 2)
    lay_pos = NodePosition() if make_distance else None
    lay_shift = ShiftPeriodicLattice() if (make_distance and crystal) else None
    lay_dist = NodeDistanceEuclidean() if make_distance else None
    lay_gauss = GaussBasisLayer(**gauss_args) if expand_distance else None
    dense0 = Dense(interaction_args["units"], activation="linear")
    interactions = [SchNetInteraction(**interaction_args) for _ in range(depth)]
    for inter in interactions:
        # a crystal receiver has more than 32 edges: the fused cfconv adds its partial rows in edge order, not with atomics
        inter.lay_cfconv.deterministic = bool(crystal)
    last = GraphMLP(**last_mlp)
    pool = PoolingNodes(**node_pooling_args) if output_embedding == "graph" else None
    out_mlp = None
    if use_output_mlp:
        out_mlp = MLP(**output_mlp) if output_embedding == "graph" else GraphMLP(**output_mlp)
    cast = ChangeTensorType(input_tensor_type="ragged", output_tensor_type="tensor") \
        if (output_embedding == "node" and output_to_tensor) else None

    def forward(model_inputs, fused=None, **kwargs):
        # Fused route (csrc/mp_schnet_node.hip, mp_cfconv.hip: stage 0, depth x (cfconv + node chain), readout = 8 kernels,
        # graph-replayed for a re-bound batch) whenever configuration and inputs fit it and no gradient is requested;
        # ``fused=False`` forces the layer path below, ``fused=True`` insists on the kernels.
        if route is not None and fused is not False and route.accepts(model_inputs):
            return route(model_inputs)
        if fused is True:
            raise ValueError("this Schnet configuration / these inputs do not fit the fused kernels")
        if crystal:
            node_input, xyz_input, edge_index_input, edge_image, lattice = model_inputs
        else:
            node_input, xyz_input, edge_index_input = model_inputs
        n = embed(node_input)
        edi = edge_index_input
        if make_distance:
            pos1, pos2 = lay_pos([xyz_input, edi])
            if crystal:
                pos2 = lay_shift([pos2, edge_image, lattice])
            ed = lay_dist([pos1, pos2])
        else:
            ed = xyz_input
        if expand_distance:
            ed = lay_gauss(ed)
        n = dense0(n)
        for inter in interactions:
            n = inter([n, ed, edi])
        n = last(n)
        if output_embedding == "graph":
            out = pool(n)
            if use_output_mlp:
                out = out_mlp(out)
        else:
            out = n
            if use_output_mlp:
                out = out_mlp(out)
            if cast is not None:
                out = cast(out)
        return out

    # Weights are created here, in the reference's construction order, so set_weights() works before a first call.
    units = interaction_args["units"]
    node_dim = input_embedding["node"]["output_dim"] if len(inputs[0]["shape"]) < 2 else inputs[0]["shape"][-1]
    edge_dim = gauss_args["bins"] if expand_distance else inputs[1]["shape"][-1]
    embed.ensure_built((None, None))
    dense0.ensure_built((None, None, node_dim))
    for inter in interactions:
        inter.ensure_built([(None, None, units), (None, None, edge_dim), (None, None, 2)])
    last.ensure_built((None, None, units))
    last_dim = last_mlp["units"][-1] if isinstance(last_mlp["units"], (list, tuple)) else last_mlp["units"]
    if out_mlp is not None:
        out_mlp.ensure_built((None, last_dim) if output_embedding == "graph" else (None, None, last_dim))
    layers = [embed, dense0] + interactions + [last] + ([out_mlp] if out_mlp is not None else [])

    def fused_tensors():
        """The model's live weight tensors under the names the fused kernels' host side uses (synth.schnet_params)."""
        p = {"embedding": embed.embeddings, "dense0/kernel": dense0.kernel, "dense0/bias": dense0.bias}
        for i, inter in enumerate(interactions):
            pre, cf = "interaction%d/" % i, inter.lay_cfconv
            p[pre + "cfconv/dense1/kernel"], p[pre + "cfconv/dense1/bias"] = cf.lay_dense1.kernel, cf.lay_dense1.bias
            p[pre + "cfconv/dense2/kernel"], p[pre + "cfconv/dense2/bias"] = cf.lay_dense2.kernel, cf.lay_dense2.bias
            p[pre + "dense1/kernel"] = inter.lay_dense1.kernel
            p[pre + "dense2/kernel"], p[pre + "dense2/bias"] = inter.lay_dense2.kernel, inter.lay_dense2.bias
            p[pre + "dense3/kernel"], p[pre + "dense3/bias"] = inter.lay_dense3.kernel, inter.lay_dense3.bias
        for name, mlp in (("last_mlp", last), ("output_mlp", out_mlp)):
            for k, d in enumerate(mlp.mlp_dense_layer_list if mlp is not None else []):
                p["%s/%d/kernel" % (name, k)], p["%s/%d/bias" % (name, k)] = d.kernel, d.bias
        return p

    merged = {"inputs": inputs, "input_embedding": input_embedding, "make_distance": make_distance,
              "expand_distance": expand_distance, "gauss_args": gauss_args, "interaction_args": interaction_args,
              "node_pooling_args": node_pooling_args, "depth": depth, "last_mlp": last_mlp,
              "output_embedding": output_embedding, "use_output_mlp": use_output_mlp, "output_mlp": output_mlp}
    route = None
    if not crystal and _fused.supports(merged) and embed.use_embedding:
        route = _fused.SchnetFusedRoute(fused_tensors, depth, gauss_args)
    model = Model(name, forward, layers, config={"depth": depth, "interaction_args": interaction_args,
                                                  "gauss_args": gauss_args, "last_mlp": last_mlp,
                                                  "output_mlp": output_mlp, "node_pooling_args": node_pooling_args,
                                                  "input_embedding": input_embedding,
                                                  "output_embedding": output_embedding},
                  auto_graph=crystal)
    model.__kgcnn_model_version__ = __model_version__
    model.fused = route   # None: this configuration always runs the layer path
    return model
