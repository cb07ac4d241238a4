"""CGCNN model builder (mirror of kgcnn/literature/CGCNN.py:22-189): Xie, Grossman, "Crystal Graph Convolutional Neural
Networks for an Accurate and Interpretable Prediction of Material Properties"
(https://journals.aps.org/prl/abstract/10.1103/PhysRevLett.120.145301).

Geometry: ``d_ij = f_i - (f_j + m_ij)`` in fractional coordinates (``DisplacementVectorsUnitCell``), taken to real space
by ``FracToRealCoordinates``, its norm expanded in a Gauss basis; then ``depth`` gated ``CGCNNLayer`` steps on a node
embedding of ``conv_layer_args["units"]`` columns, node pooling and the output MLP.

**The lattice convention.**  The reference's ``FracToRealCoordinates`` computes ``A f`` (einsum ``'ij,ikj->ik'``), not the
``f A`` with lattice vectors in rows of its docstring.  The code is mirrored, so a ``graph_lattice`` in the row convention
(pymatgen, ``SetRangePeriodic``) has to be passed to this model **transposed**: ``lattice.transpose(1, 2).contiguous()``.
``SetRangePeriodic`` output feeds the model otherwise as it is: ``range_indices`` are the edges, ``range_image`` (int64,
cast here) the ``cell_translations``; fractional coordinates are the caller's.

``model.weights`` order: ``node embedding`` (``embeddings``, with an embedding input), the input ``Dense`` (``kernel,
bias``), per ``CGCNNLayer`` with batch normalisation ``batch_norm_f``, ``batch_norm_s``, ``batch_norm_out`` (each
``gamma, beta, moving_mean, moving_variance``) and then ``f``, ``s`` (each ``kernel, bias``), last the output MLP.  Keras
lists the non-trainable statistics after ALL trainable weights of the model, so a batch-normalised Keras weight list has to
be reordered before ``set_weights``.

A layer whose sizes fit ``layers/conv/cgcnn_conv.py`` (width 64, at most 64 edge features, sum pooling) runs on the fused
``mp_cgcnn_gate_f32``; every other configuration, every call on a tape and ``layer.use_fused_gate = False`` (or
``model.use_fused_gate = False`` for all layers) take the layer sequence.  Batch normalisation runs in inference mode
only: ``train_on_batch`` / ``fit`` of a batch-normalised model raise ``NotImplementedError``; with
``batch_normalization=False`` the model trains through the existing rules.  ``representation="asu"`` is not built.
"""
import torch

from ..layers.conv.cgcnn_conv import CGCNNLayer
from ..layers.geom import (DisplacementVectorsUnitCell, EuclideanNorm, FracToRealCoordinates, GaussBasisLayer,
                           NodePosition)
from ..layers.mlp import MLP
from ..layers.modules import Dense, LazySubtract, OptionalInputEmbedding
from ..layers.pooling import PoolingNodes
from ..model.utils import RouteSwitchModel, update_model_kwargs
from ..ragged import RaggedTensor

__model_version__ = "2022.11.25"

model_crystal_default = {
    "name": "CGCNN",
    "inputs": [
        {"shape": (None,), "name": "node_number", "dtype": "int64", "ragged": True},
        {"shape": (None, 3), "name": "node_frac_coordinates", "dtype": "float64", "ragged": True},
        {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
        {"shape": (3, 3), "name": "lattice_matrix", "dtype": "float64", "ragged": False},
        {"shape": (None, 3), "name": "cell_translations", "dtype": "float32", "ragged": True},
    ],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64}},
    "representation": "unit",  # None, "asu" or "unit"
    "expand_distance": True,
    "make_distances": True,
    "gauss_args": {"bins": 40, "distance": 8, "offset": 0.0, "sigma": 0.4},
    "depth": 3,
    "verbose": 10,
    "conv_layer_args": {
        "units": 64,
        "activation_s": "softplus",
        "activation_out": "softplus",
        "batch_normalization": True,
    },
    "node_pooling_args": {"pooling_method": "mean"},
    "output_embedding": "graph",
    "output_mlp": {"use_bias": [True, False], "units": [64, 1],
                   "activation": ["softplus", "linear"]},
}


class _CgcnnModel(RouteSwitchModel):
    """``Model`` with the ``use_fused_gate`` switch over all layers."""

    switch_attr, switch_layers_attr = "use_fused_gate", "conv_layers"
    conv_layers = ()
    use_fused_gate = RouteSwitchModel.switch


def _float32(x):
    """float64 coordinates / lattices are cast once at the model's entry: the engine computes in float32."""
    if isinstance(x, RaggedTensor):
        return x.with_values(x.values.to(torch.float32)) if x.values.dtype == torch.float64 else x
    return x.to(torch.float32) if torch.is_tensor(x) and x.dtype == torch.float64 else x


@update_model_kwargs(model_crystal_default)
def make_crystal_model(inputs: list = None, representation: str = None, make_distances: bool = None,
                       input_embedding: dict = None, conv_layer_args: dict = None, expand_distance: bool = None,
                       depth: int = None, name: str = None, verbose: int = None, gauss_args: dict = None,
                       node_pooling_args: dict = None, output_mlp: dict = None, output_embedding: str = None):
    r"""Build CGCNN (kgcnn/literature/CGCNN.py:54-189).  Model inputs

    * ``[node_attributes, node_frac_coordinates, edge_indices, lattice, cell_translations]`` with
      ``representation="unit"`` (the default);
    * ``[node_attributes, node_frac_coordinates, edge_indices, lattice]`` with ``representation=None``;
    * ``[node_attributes, edge_distance, edge_indices]`` with ``make_distances=False`` (``edge_distance``
      ``(batch, [M], 1)`` with ``expand_distance=True``, else the ``(batch, [M], D)`` edge features themselves).

    ``lattice`` is a dense ``(batch, 3, 3)`` tensor.  **It enters as** ``A f``: a lattice with its vectors in rows
    (pymatgen, ``SetRangePeriodic``) has to be passed transposed - see the module docstring.  ``cell_translations`` may be
    the int64 ``range_image`` of ``SetRangePeriodic``.  float64 coordinates and lattices are cast to float32.  Output:
    ``(batch, L)`` graph embeddings.  ``model.fused_gate_layers`` lists which layers fit the fused kernel;
    ``model.conv_layers[i].use_fused_gate`` / ``model.use_fused_gate`` switch it."""
    if output_embedding != "graph":
        raise ValueError("Unsupported output embedding for mode `CGCNN`.")
    if representation == "asu":
        raise NotImplementedError("CGCNN with representation='asu' (DisplacementVectorsASU, symmetry operations) is not "
                                  "implemented")
    if representation not in (None, "unit"):
        raise ValueError("representation must be None, 'unit' or 'asu', got %r" % (representation,))
    lay_disp = lay_pos = lay_sub = lay_real = lay_norm = None
    if make_distances:
        if representation == "unit":
            lay_disp = DisplacementVectorsUnitCell()
        else:
            lay_pos, lay_sub = NodePosition(), LazySubtract()
        lay_real = FracToRealCoordinates()
        lay_norm = EuclideanNorm(axis=2, keepdims=True)
    lay_gauss = GaussBasisLayer(**gauss_args) if expand_distance else None
    embed_n = OptionalInputEmbedding(**input_embedding["node"], use_embedding=len(inputs[0]["shape"]) < 2)
    dense_in = Dense(conv_layer_args["units"], activation="linear")
    convs = [CGCNNLayer(**conv_layer_args) for _ in range(depth)]
    pool = PoolingNodes(**node_pooling_args)
    out_mlp = MLP(**output_mlp)

    # weights exist before the first call (set_weights / get_weights); widths follow the op sequence
    h0_dim = input_embedding["node"]["output_dim"] if embed_n.use_embedding else inputs[0]["shape"][-1]
    if expand_distance:
        edge_dim = int(gauss_args["bins"]) if "bins" in gauss_args else lay_gauss.bins
    else:
        edge_dim = 1 if make_distances else inputs[1]["shape"][-1]
    units = conv_layer_args["units"]
    embed_n.ensure_built((None, None))
    dense_in.ensure_built((None, None, h0_dim))
    for lay in convs:
        lay.ensure_built([(None, None, units), (None, None, edge_dim), (None, None, 2)])
    out_mlp.ensure_built((None, units))

    def forward(model_inputs, **kwargs):
        if make_distances:
            want = 5 if representation == "unit" else 4
            if len(model_inputs) < want:
                raise ValueError("CGCNN expects [node_attributes, node_frac_coordinates, edge_indices, lattice%s]"
                                 % (", cell_translations" if want == 5 else ""))
            node_input, edi = model_inputs[0], model_inputs[2]
            frac, lattice = _float32(model_inputs[1]), _float32(model_inputs[3])
            if representation == "unit":
                disp = lay_disp([frac, edi, model_inputs[4]], **kwargs)
            else:
                x_in, x_out = lay_pos([frac, edi], **kwargs)
                disp = lay_sub([x_out, x_in], **kwargs)
            disp = lay_real([disp, lattice], **kwargs)
            ed = lay_norm(disp, **kwargs)
        else:
            node_input, ed, edi = model_inputs[0], _float32(model_inputs[1]), model_inputs[2]
        if lay_gauss is not None:
            ed = lay_gauss(ed, **kwargs)
        n = dense_in(embed_n(node_input, **kwargs), **kwargs)
        for lay in convs:
            n = lay([n, ed, edi], **kwargs)
        return out_mlp(pool(n, **kwargs), **kwargs)

    layers = [embed_n, dense_in] + convs + [out_mlp]
    config = {"inputs": inputs, "representation": representation, "make_distances": make_distances,
              "input_embedding": input_embedding, "conv_layer_args": conv_layer_args,
              "expand_distance": expand_distance, "depth": depth, "gauss_args": gauss_args,
              "node_pooling_args": node_pooling_args, "output_mlp": output_mlp, "output_embedding": output_embedding}
    model = _CgcnnModel(name, forward, layers, config=config)
    model.__kgcnn_model_version__ = __model_version__
    model.fused = None
    model.conv_layers = convs
    model.fused_gate_layers = [bool(lay.fused_gate) for lay in convs]
    # the layer sequence is replayed from one HIP graph for re-bound inputs (model/utils.py)
    model.auto_graph = True
    return model
