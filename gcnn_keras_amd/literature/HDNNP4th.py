"""HDNNP4th model builders (mirror of kgcnn/literature/HDNNP4th.py:1-445): the fourth-generation high-dimensional neural
network potential of Ko, Finkler, Goedecker and Behler (2021).  ACSF G2 + G4 with the QM/MM electrostatic potential
appended, an element-keyed ``RelationalMLP`` for the electronegativities, CENT charge equilibration with the
Gaussian-charge electrostatic energy (``CENTChargePlusElectrostaticEnergy``, csrc/mp_cent.hip), the QM/MM point-charge
energy and a second ``RelationalMLP`` for the short-range atomic energies on ``[representation, esp, charge]``.

A model's ``weights`` / ``set_weights`` hold the layers on its output's path, as a Keras functional model does: the
``"charge"`` and ``"electrostatic_energy"`` models the charge MLP only, the energy models the charge MLP, then the local
MLP.  A truthy ``normalize_kwargs`` (``GraphBatchNormalization``) raises ``NotImplementedError``.
"""
from ..layers.casting import ChangeTensorType
from ..layers.conv.acsf_conv import ACSFG2, ACSFG4
from ..layers.conv.hdnnp_conv import CENTChargePlusElectrostaticEnergy, ElectrostaticQMMMEnergyPointCharge
from ..layers.mlp import MLP, RelationalMLP
from ..layers.modules import ExpandDims, LazyAdd, LazyConcatenate
from ..layers.pooling import PoolingNodes
from ..model.utils import Model, update_model_kwargs
from .HDNNP2nd import _mapping

__model_version__ = "2023.02.17"

_INPUTS = [{"shape": (None,), "name": "node_number", "dtype": "int64", "ragged": True},
           {"shape": (None, 3), "name": "node_coordinates", "dtype": "float32", "ragged": True},
           {"shape": (None, 2), "name": "range_indices", "dtype": "int64", "ragged": True},
           {"shape": (None, 3), "name": "angle_indices_nodes", "dtype": "int64", "ragged": True},
           {"shape": (1,), "name": "total_charge", "dtype": "float32", "ragged": False},
           {"shape": (None,), "name": "esp", "dtype": "float32", "ragged": True},
           {"shape": (None, 3), "name": "esp_grad", "dtype": "float32", "ragged": True}]

# The reference's defaults list the first five inputs; its builders read seven (the fork passes all of them).
model_default_behler = {
    "name": "HDNNP4th",
    "inputs": _INPUTS,
    "g2_kwargs": {"eta": [0.0, 0.3], "rs": [0.0, 3.0], "rc": 10.0, "elements": [1, 6, 16]},
    "g4_kwargs": {"eta": [0.0, 0.3], "lamda": [-1.0, 1.0], "rc": 6.0,
                  "zeta": [1.0, 8.0], "elements": [1, 6, 16], "multiplicity": 2.0},
    "normalize_kwargs": {},
    "mlp_charge_kwargs": {"units": [64, 64, 1],
                          "num_relations": 96,
                          "activation": ["swish", "swish", "linear"]},
    "mlp_local_kwargs": {"units": [64, 64, 1],
                         "num_relations": 96,
                         "activation": ["swish", "swish", "linear"]},
    "cent_kwargs": {},
    "electrostatic_kwargs": {"name": "electrostatic_layer",
                             "use_physical_params": True,
                             "param_trainable": False},
    "qmmm_kwargs": {"name": "qmmm_layer"},
    "node_pooling_args": {"pooling_method": "sum"},
    "verbose": 10,
    "output_embedding": "graph",
    "output_to_tensor": True,
    "use_output_mlp": False,
    "output_mlp": {"use_bias": [True, True], "units": [64, 1],
                   "activation": ["swish", "linear"]},
    "energy_mean_and_var": None
}

_EMBEDDINGS = ("graph", "total_energy", "charge", "electrostatic_energy", "charge+qm_energy")


class _PaddedCharges(ChangeTensorType):
    """``q.to_tensor()`` (HDNNP4th.py:167): the padded charges ``(batch, Nmax, 1)``; on the tape (``autograd.RaggedToPadded``)
    when the charges require grad, so that a loss on them trains the charge network."""

    weight_gradients = True

    def __init__(self, **kwargs):
        super().__init__(input_tensor_type="ragged", output_tensor_type="tensor", **kwargs)

    def call(self, inputs, **kwargs):
        from ..autograd import RaggedToPadded, needs_grad
        if needs_grad(inputs.values):
            return RaggedToPadded.apply(inputs.values, inputs.row_splits, inputs.row_splits_host())
        return super().call(inputs, **kwargs)


def _check(g2_kwargs, g4_kwargs, mlp_charge_kwargs, mlp_local_kwargs, normalize_kwargs):
    for mlp_name, mlp_kwargs in (("mlp_charge_kwargs", mlp_charge_kwargs), ("mlp_local_kwargs", mlp_local_kwargs)):
        if mlp_kwargs is None:
            continue
        for g_name, g_kwargs in (("g2_kwargs", g2_kwargs), ("g4_kwargs", g4_kwargs)):
            if g_kwargs is not None:
                assert max(_mapping(g_kwargs)) < mlp_kwargs.get("num_relations"), \
                    "Elemental mapping in %s exceeds num_relations in %s." % (g_name, mlp_name)
    if normalize_kwargs:
        raise NotImplementedError("normalize_kwargs (GraphBatchNormalization) is not implemented for HDNNP4th")


def _acsf(g2_kwargs, g4_kwargs):
    g2_table = {k: v for k, v in g2_kwargs.items() if k != "elemental_mapping"}
    g4_table = {k: v for k, v in g4_kwargs.items() if k != "elemental_mapping"}
    return ACSFG2(**ACSFG2.make_param_table(**g2_table)), ACSFG4(**ACSFG4.make_param_table(**g4_table))


class _Network:
    """The layers shared by the builders, from ``rep_esp`` on (HDNNP4th.py:144-168): one instance per builder call, so
    that ``make_model_behler_charge_separat``'s two models share them."""

    def __init__(self, width, mlp_charge_kwargs, mlp_local_kwargs, cent_kwargs, electrostatic_kwargs, qmmm_kwargs,
                 node_pooling_args):
        self.expand = ExpandDims(axis=2)
        self.concat_esp = LazyConcatenate(axis=2)
        self.mlp_charge = RelationalMLP(**mlp_charge_kwargs)
        self.add_esp = LazyAdd()
        self.cent = CENTChargePlusElectrostaticEnergy(**cent_kwargs, **electrostatic_kwargs)
        self.qmmm = ElectrostaticQMMMEnergyPointCharge(**qmmm_kwargs)
        self.concat_q = LazyConcatenate(axis=2)
        self.mlp_local = RelationalMLP(**mlp_local_kwargs)
        self.pool = PoolingNodes(**node_pooling_args)
        self.add_total = LazyAdd()
        self.cast = _PaddedCharges()
        self.mlp_charge.ensure_built([(None, None, width + 1), (None, None)])
        self.mlp_local.ensure_built([(None, None, width + 2), (None, None)])

    def charge_layers(self):
        return [self.expand, self.concat_esp, self.mlp_charge, self.add_esp, self.cent]

    def energy_layers(self):
        return self.charge_layers() + [self.qmmm, self.concat_q, self.mlp_local, self.pool, self.add_total]

    def charges(self, rep, z, xyz, ij, qtot, esp, **kwargs):
        """(esp (batch, [N], 1), rep_esp, q (batch, [N], 1), E_elec (batch, 1))."""
        esp_e = self.expand(esp)
        rep_esp = self.concat_esp([rep, esp_e])
        chi = self.mlp_charge([rep_esp, z], **kwargs)
        q, e_elec = self.cent([z, self.add_esp([chi, esp_e]), xyz, ij, qtot])
        return rep_esp, q, e_elec

    def energy(self, rep_esp, z, q, e_elec, esp, **kwargs):
        e_qmmm = self.qmmm([q, esp])
        local = self.mlp_local([self.concat_q([rep_esp, q]), z], **kwargs)
        return self.add_total([self.pool(local), e_elec, e_qmmm])


def _model(name, forward, layers, config):
    model = Model(name, forward, layers, config=config)
    model.__kgcnn_model_version__ = __model_version__
    model.fused = None
    # the layer sequence is replayed from one HIP graph for re-bound inputs (model/utils.py)
    model.auto_graph = True
    return model


def _output_mlp(output_embedding, use_output_mlp, output_mlp):
    if use_output_mlp and output_embedding in ("graph", "total_energy"):
        mlp = MLP(**output_mlp)
        mlp.ensure_built((None, 1))
        return mlp
    return None


@update_model_kwargs(model_default_behler)
def make_model_behler(inputs: list = None, node_pooling_args: dict = None, name: str = None, verbose: int = None,
                      normalize_kwargs: dict = None, g2_kwargs: dict = None, g4_kwargs: dict = None,
                      mlp_charge_kwargs: dict = None, mlp_local_kwargs: dict = None, cent_kwargs: dict = None,
                      electrostatic_kwargs: dict = None, qmmm_kwargs: dict = None, output_embedding: str = None,
                      use_output_mlp: bool = None, output_to_tensor: bool = None, output_mlp: dict = None,
                      energy_mean_and_var: tuple = None):
    r"""Build HDNNP4th (kgcnn/literature/HDNNP4th.py:59-189).  Model inputs ``[node_number, node_coordinates,
    range_indices (.., 2), angle_indices_nodes (.., 3), total_charge (batch, 1), esp (batch, [N]), esp_grad
    (batch, [N], 3)]``; ``esp_grad`` is not read by the model (``EnergyForceModel`` consumes it).  ``output_embedding``:
    ``"graph"`` / ``"total_energy"`` (the total energy, with ``use_output_mlp``), ``"charge"`` (padded charges
    ``(batch, Nmax, 1)``), ``"electrostatic_energy"`` or ``"charge+qm_energy"`` (``[charges padded, total energy]``)."""
    _check(g2_kwargs, g4_kwargs, mlp_charge_kwargs, mlp_local_kwargs, normalize_kwargs)
    if output_embedding not in _EMBEDDINGS:
        raise ValueError("Unsupported output embedding for mode `HDNNP4th`")
    g2, g4 = _acsf(g2_kwargs, g4_kwargs)
    concat = LazyConcatenate()
    width = g2.num_relations * g2.num_functions + g4.num_relations * g4.num_functions
    net = _Network(width, mlp_charge_kwargs, mlp_local_kwargs, cent_kwargs, electrostatic_kwargs, qmmm_kwargs,
                   node_pooling_args)
    out_mlp = _output_mlp(output_embedding, use_output_mlp, output_mlp)

    def forward(model_inputs, **kwargs):
        z, xyz, ij, ijk, qtot, esp = model_inputs[:6]
        rep = concat([g2([z, xyz, ij]), g4([z, xyz, ijk])])
        rep_esp, q, e_elec = net.charges(rep, z, xyz, ij, qtot, esp, **kwargs)
        if output_embedding == "charge":
            return net.cast(q)
        if output_embedding == "electrostatic_energy":
            return e_elec
        e = net.energy(rep_esp, z, q, e_elec, esp, **kwargs)
        if output_embedding == "charge+qm_energy":
            return [net.cast(q), e]
        return out_mlp(e) if out_mlp is not None else e

    path = net.charge_layers() if output_embedding in ("charge", "electrostatic_energy") else net.energy_layers()
    layers = [g2, g4, concat] + path + [net.cast] + ([out_mlp] if out_mlp is not None else [])
    return _model(name, forward, layers, {"g2_kwargs": g2_kwargs, "g4_kwargs": g4_kwargs,
                                          "mlp_charge_kwargs": mlp_charge_kwargs, "mlp_local_kwargs": mlp_local_kwargs,
                                          "output_embedding": output_embedding})


@update_model_kwargs(model_default_behler)
def make_model_behler_charge_separat(inputs: list = None, node_pooling_args: dict = None, name: str = None,
                                     verbose: int = None, normalize_kwargs: dict = None, g2_kwargs: dict = None,
                                     g4_kwargs: dict = None, mlp_charge_kwargs: dict = None,
                                     mlp_local_kwargs: dict = None, cent_kwargs: dict = None,
                                     electrostatic_kwargs: dict = None, qmmm_kwargs: dict = None,
                                     output_embedding: str = None, use_output_mlp: bool = None,
                                     output_to_tensor: bool = None, output_mlp: dict = None,
                                     energy_mean_and_var: tuple = None):
    r"""``(model_charge, model_energy)`` sharing their layers (kgcnn/literature/HDNNP4th.py:191-313): ``model_charge``
    returns the padded charges, ``model_energy`` the ``output_embedding`` (``"graph"`` / ``"total_energy"``, ``"charge"``
    - the ragged charges, as in the reference - or ``"charge+qm_energy"``)."""
    _check(g2_kwargs, g4_kwargs, mlp_charge_kwargs, mlp_local_kwargs, normalize_kwargs)
    if output_embedding not in ("graph", "total_energy", "charge", "charge+qm_energy"):
        raise ValueError("Unsupported output embedding for mode `HDNNP4th`")
    g2, g4 = _acsf(g2_kwargs, g4_kwargs)
    concat = LazyConcatenate()
    width = g2.num_relations * g2.num_functions + g4.num_relations * g4.num_functions
    net = _Network(width, mlp_charge_kwargs, mlp_local_kwargs, cent_kwargs, electrostatic_kwargs, qmmm_kwargs,
                   node_pooling_args)
    out_mlp = _output_mlp(output_embedding, use_output_mlp, output_mlp)

    def charges(model_inputs, **kwargs):
        z, xyz, ij, ijk, qtot, esp = model_inputs[:6]
        rep = concat([g2([z, xyz, ij]), g4([z, xyz, ijk])])
        return (z, xyz, esp) + net.charges(rep, z, xyz, ij, qtot, esp, **kwargs)

    def forward_charge(model_inputs, **kwargs):
        return net.cast(charges(model_inputs, **kwargs)[4])

    def forward_energy(model_inputs, **kwargs):
        z, xyz, esp, rep_esp, q, e_elec = charges(model_inputs, **kwargs)
        if output_embedding == "charge":
            return q
        e = net.energy(rep_esp, z, q, e_elec, esp, **kwargs)
        if output_embedding == "charge+qm_energy":
            return [net.cast(q), e]
        return out_mlp(e) if out_mlp is not None else e

    config = {"g2_kwargs": g2_kwargs, "g4_kwargs": g4_kwargs, "mlp_charge_kwargs": mlp_charge_kwargs,
              "mlp_local_kwargs": mlp_local_kwargs, "output_embedding": output_embedding}
    model_charge = _model(name, forward_charge, [g2, g4, concat] + net.charge_layers() + [net.cast], config)
    path = net.charge_layers() if output_embedding == "charge" else net.energy_layers()
    model_energy = _model(name, forward_energy,
                          [g2, g4, concat] + path + [net.cast] + ([out_mlp] if out_mlp is not None else []), config)
    return model_charge, model_energy


def make_model_rep(inputs: list = None, name: str = None, verbose: int = None, g2_kwargs: dict = None,
                   g4_kwargs: dict = None):
    r"""The ACSF representation alone (kgcnn/literature/HDNNP4th.py:315-335): inputs ``[node_number,
    node_coordinates, range_indices, angle_indices_nodes]``, output ``concat(G2, G4)`` ``(batch, [N], F)``."""
    g2, g4 = _acsf(g2_kwargs, g4_kwargs)
    concat = LazyConcatenate()

    def forward(model_inputs, **kwargs):
        z, xyz, ij, ijk = model_inputs[:4]
        return concat([g2([z, xyz, ij]), g4([z, xyz, ijk])])

    return _model(name or "HDNNP4th", forward, [g2, g4, concat], {"g2_kwargs": g2_kwargs, "g4_kwargs": g4_kwargs})


def make_model_learn(inputs: list = None, node_pooling_args: dict = None, name: str = None, verbose: int = None,
                     normalize_kwargs: dict = None, mlp_charge_kwargs: dict = None, mlp_local_kwargs: dict = None,
                     cent_kwargs: dict = None, electrostatic_kwargs: dict = None, qmmm_kwargs: dict = None,
                     output_embedding: str = None, use_output_mlp: bool = None, output_to_tensor: bool = None,
                     output_mlp: dict = None):
    r"""HDNNP4th on a representation computed in advance by ``make_model_rep`` (kgcnn/literature/HDNNP4th.py:337-445):
    inputs ``[node_number, node_coordinates, range_indices, angle_indices_nodes, total_charge, rep (batch, [N], F),
    esp (batch, [N])]``; ``output_embedding`` must be ``"graph"`` (the total energy, with ``use_output_mlp``)."""
    _check(None, None, mlp_charge_kwargs, mlp_local_kwargs, normalize_kwargs)
    if output_embedding != "graph":
        raise ValueError("Unsupported output embedding for mode `HDNNP4th`")
    width = int(inputs[5]["shape"][-1])
    net = _Network(width, mlp_charge_kwargs, mlp_local_kwargs, cent_kwargs or {}, electrostatic_kwargs or {},
                   qmmm_kwargs or {}, node_pooling_args or {"pooling_method": "sum"})
    out_mlp = _output_mlp(output_embedding, use_output_mlp, output_mlp)

    def forward(model_inputs, **kwargs):
        z, xyz, ij, _, qtot, rep, esp = model_inputs[:7]
        rep_esp, q, e_elec = net.charges(rep, z, xyz, ij, qtot, esp, **kwargs)
        e = net.energy(rep_esp, z, q, e_elec, esp, **kwargs)
        return out_mlp(e) if out_mlp is not None else e

    layers = net.energy_layers() + ([out_mlp] if out_mlp is not None else [])
    return _model(name or "HDNNP4th", forward, layers, {"mlp_charge_kwargs": mlp_charge_kwargs,
                                                        "mlp_local_kwargs": mlp_local_kwargs})
