"""HDNNP2nd model builders (mirror of kgcnn/literature/HDNNP2nd.py:1-419): Behler's second-generation high-dimensional
neural network potential - atom-centred symmetry functions (``ACSFG2``, ``ACSFG4``), concatenated, an element-keyed
``RelationalMLP`` per atom and a sum over the atoms.

``make_model_behler`` and ``make_model_atom_wise`` are built; the weighted-ACSF (``make_model_weighted``, wACSF) and
inverse-distance builders raise ``NotImplementedError``, and so does a truthy ``normalize_kwargs``
(``GraphBatchNormalization``).  ``make_model`` is ``make_model_weighted``, as in the reference.
"""
from ..layers.casting import ChangeTensorType
from ..layers.conv.acsf_conv import ACSFG2, ACSFG4
from ..layers.mlp import MLP, GraphMLP, RelationalMLP
from ..layers.modules import LazyConcatenate
from ..layers.pooling import PoolingNodes
from ..model.utils import Model, update_model_kwargs

__model_version__ = "2023.01.17"

model_default_behler = {
    "name": "HDNNP2nd",
    "inputs": [{"shape": (None,), "name": "node_number", "dtype": "int64", "ragged": True},
               {"shape": (None, 3), "name": "node_coordinates", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "range_indices", "dtype": "int64", "ragged": True},
               {"shape": (None, 3), "name": "angle_indices_nodes", "dtype": "int64", "ragged": True}],
    "g2_kwargs": {"eta": [0.0, 0.3], "rs": [0.0, 3.0], "rc": 10.0, "elements": [1, 6, 16]},
    "g4_kwargs": {"eta": [0.0, 0.3], "lamda": [-1.0, 1.0], "rc": 6.0,
                  "zeta": [1.0, 8.0], "elements": [1, 6, 16], "multiplicity": 2.0},
    "normalize_kwargs": {},
    "mlp_kwargs": {"units": [64, 64, 1],
                   "num_relations": 96,
                   "activation": ["swish", "swish", "linear"]},
    "node_pooling_args": {"pooling_method": "sum"},
    "verbose": 10,
    "output_embedding": "graph", "output_to_tensor": True,
    "use_output_mlp": False,
    "output_mlp": {"use_bias": [True, True], "units": [64, 1],
                   "activation": ["swish", "linear"]}
}

model_atom_wise_default = {
    "name": "HDNNP2nd",
    "inputs": [{"shape": (None,), "name": "node_number", "dtype": "int64", "ragged": True},
               {"shape": (None, 3), "name": "node_representation", "dtype": "float32", "ragged": True}],
    "mlp_kwargs": {"units": [64, 64, 1],
                   "num_relations": 96,
                   "activation": ["swish", "swish", "linear"]},
    "node_pooling_args": {"pooling_method": "sum"},
    "verbose": 10,
    "output_embedding": "graph", "output_to_tensor": True,
    "use_output_mlp": False,
    "output_mlp": {"use_bias": [True, True], "units": [64, 1],
                   "activation": ["swish", "linear"]}
}


def _mapping(kwargs):
    """The elements a symmetry-function table covers (``elemental_mapping`` when given, else ``elements``)."""
    return kwargs.get("elemental_mapping", kwargs.get("elements"))


def _readout(n, pool, out_mlp, cast, output_embedding):
    if output_embedding == "graph":
        out = pool(n)
        return out_mlp(out) if out_mlp is not None else out
    out = out_mlp(n) if out_mlp is not None else n
    return cast(out) if cast is not None else out


def _readout_layers(output_embedding, node_pooling_args, use_output_mlp, output_to_tensor, output_mlp):
    if output_embedding not in ("graph", "node"):
        raise ValueError("Unsupported output embedding for mode `HDNNP2nd`")
    pool = PoolingNodes(**node_pooling_args) if output_embedding == "graph" else None
    out_mlp = None
    if use_output_mlp:
        out_mlp = MLP(**output_mlp) if output_embedding == "graph" else GraphMLP(**output_mlp)
    cast = ChangeTensorType(input_tensor_type="ragged", output_tensor_type="tensor") \
        if (output_embedding == "node" and output_to_tensor) else None
    return pool, out_mlp, cast


def _build_readout(pool, out_mlp, units, output_embedding):
    if out_mlp is not None:
        out_mlp.ensure_built((None, units) if output_embedding == "graph" else (None, None, units))
    return [layer for layer in (pool, out_mlp) if layer is not None]


@update_model_kwargs(model_default_behler)
def make_model_behler(inputs: list = None, node_pooling_args: dict = None, name: str = None, verbose: int = None,
                      normalize_kwargs: dict = None, g2_kwargs: dict = None, g4_kwargs: dict = None,
                      mlp_kwargs: dict = None, output_embedding: str = None, use_output_mlp: bool = None,
                      output_to_tensor: bool = None, output_mlp: dict = None):
    r"""Build HDNNP2nd with Behler's ACSF (kgcnn/literature/HDNNP2nd.py:154-242).  Model inputs ``[node_number,
    node_coordinates, range_indices (.., 2), angle_indices_nodes (.., 3)]``."""
    assert max(_mapping(g2_kwargs)) < mlp_kwargs.get("num_relations"), \
        "Elemental mapping in g2_kwargs exceeds num_relations in mlp_kwargs."
    assert max(_mapping(g4_kwargs)) < mlp_kwargs.get("num_relations"), \
        "Elemental mapping in g4_kwargs exceeds num_relations in mlp_kwargs."
    if normalize_kwargs:
        raise NotImplementedError("normalize_kwargs (GraphBatchNormalization) is not implemented for HDNNP2nd")
    g2_table = {k: v for k, v in g2_kwargs.items() if k != "elemental_mapping"}
    g4_table = {k: v for k, v in g4_kwargs.items() if k != "elemental_mapping"}
    g2 = ACSFG2(**ACSFG2.make_param_table(**g2_table))
    g4 = ACSFG4(**ACSFG4.make_param_table(**g4_table))
    concat = LazyConcatenate()
    mlp = RelationalMLP(**mlp_kwargs)
    pool, out_mlp, cast = _readout_layers(output_embedding, node_pooling_args, use_output_mlp, output_to_tensor,
                                          output_mlp)

    def forward(model_inputs, **kwargs):
        node_input, xyz_input, edge_index_input, angle_index_input = model_inputs
        rep_g2 = g2([node_input, xyz_input, edge_index_input])
        rep_g4 = g4([node_input, xyz_input, angle_index_input])
        rep = concat([rep_g2, rep_g4])
        n = mlp([rep, node_input], **kwargs)
        return _readout(n, pool, out_mlp, cast, output_embedding)

    width = g2.num_relations * g2.num_functions + g4.num_relations * g4.num_functions
    mlp.ensure_built([(None, None, width), (None, None)])
    layers = [g2, g4, concat, mlp] + _build_readout(pool, out_mlp, mlp._conf_units[-1], output_embedding)
    model = Model(name, forward, layers, config={"g2_kwargs": g2_kwargs, "g4_kwargs": g4_kwargs,
                                                 "mlp_kwargs": mlp_kwargs})
    model.__kgcnn_model_version__ = __model_version__
    model.fused = None
    # the layer sequence is replayed from one HIP graph for re-bound inputs (model/utils.py)
    model.auto_graph = True
    return model


@update_model_kwargs(model_atom_wise_default)
def make_model_atom_wise(inputs: list = None, node_pooling_args: dict = None, name: str = None, verbose: int = None,
                         mlp_kwargs: dict = None, output_embedding: str = None, use_output_mlp: bool = None,
                         output_to_tensor: bool = None, output_mlp: dict = None):
    r"""HDNNP2nd on a given atomic representation (kgcnn/literature/HDNNP2nd.py:261-325).  Model inputs
    ``[node_number, node_representation (.., F)]``."""
    mlp = RelationalMLP(**mlp_kwargs)
    pool, out_mlp, cast = _readout_layers(output_embedding, node_pooling_args, use_output_mlp, output_to_tensor,
                                          output_mlp)

    def forward(model_inputs, **kwargs):
        node_input, rep_input = model_inputs
        n = mlp([rep_input, node_input], **kwargs)
        return _readout(n, pool, out_mlp, cast, output_embedding)

    mlp.ensure_built([(None, None, inputs[1]["shape"][-1]), (None, None)])
    layers = [mlp] + _build_readout(pool, out_mlp, mlp._conf_units[-1], output_embedding)
    model = Model(name, forward, layers, config={"mlp_kwargs": mlp_kwargs})
    model.__kgcnn_model_version__ = __model_version__
    model.fused = None
    model.auto_graph = True
    return model


def make_model_weighted(**kwargs):
    """Weighted ACSF (wACSF, kgcnn/literature/HDNNP2nd.py:46-129) is not implemented; use ``make_model_behler``."""
    raise NotImplementedError("HDNNP2nd with weighted ACSF (make_model_weighted, wACSF) is not implemented; "
                              "use make_model_behler")


def make_model_inverse_distances(**kwargs):
    """The inverse-distance variant (kgcnn/literature/HDNNP2nd.py:344-415) is not implemented; use
    ``make_model_behler``."""
    raise NotImplementedError("HDNNP2nd on inverse distances (make_model_inverse_distances) is not implemented; "
                              "use make_model_behler")


# As in the reference, the default builder is the weighted-ACSF one.
make_model = make_model_weighted
