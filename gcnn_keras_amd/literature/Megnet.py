"""MEGNet model builders (mirror of kgcnn/literature/Megnet.py:24-373, ``make_model`` and ``make_crystal_model``).

``make_model``: inputs ``[node_attributes, node_coordinates | edge_distance, edge_indices, graph_attributes]``; three
MEGNet blocks with feed-forward MLPs and skip connections, Set2Set readouts of nodes and edges, output MLP on ``[nodes |
edges | state]``.  Weights are created in construction order (embeddings, first feed-forward triple, then per block:
[feed-forward triple,] block; the two Dense + Set2Set readouts; output MLP).

``make_crystal_model`` is the periodic variant: inputs ``[node_attributes, node_coordinates | edge_distance,
edge_indices, state_attributes, edge_image, graph_lattice]``, the last a dense ``(batch, 3, 3)`` tensor with the lattice
vectors in ROWS (unlike CGCNN's ``A f``); the sender position of every edge is shifted by ``edge_image @ lattice``
(``ShiftPeriodicLattice``) before the distance is taken.  ``SetRangePeriodic`` output feeds the model as it is:
``range_indices`` are the edges, ``range_image`` (int64) the ``edge_image``, the lattice goes in untransposed.  Same
layers and weight order as ``make_model``; the state input is ``charge`` of shape ``[1]``, a float ``(batch, 1)`` tensor
(or ``(batch,)`` numbers through the embedding with ``shape: []``).

A block whose sizes fit ``layers/conv/megnet_conv.py`` (widths 32 / 32 / 32 behind the feed-forward MLPs, ``edge_embed``
``[64, 32, 32]``, mean or sum pooling) runs its edge update on the fused ``mp_megnet_edge_f32``
(``model.fused_edge_blocks``); every other configuration, every call on a tape and ``block.use_fused_edge = False`` (or
``model.use_fused_edge = False`` for all blocks) take the layer sequence.  Both builders train with
``use_set2set=False`` (``compile`` / ``train_on_batch`` / ``fit``); with ``use_set2set=True`` training raises
``NotImplementedError`` from ``PoolingSet2Set``, which has no LSTM reverse.  Dropout is not built."""
from ..layers.conv.megnet_conv import MEGnetBlock
from ..layers.geom import GaussBasisLayer, NodeDistanceEuclidean, NodePosition, ShiftPeriodicLattice
from ..layers.mlp import MLP, GraphMLP
from ..layers.modules import Dense, LazyAdd, OptionalInputEmbedding, binary_values, concat_last
from ..layers.pool.set2set import PoolingSet2Set
from ..layers.pooling import PoolingGlobalEdges, PoolingNodes
from ..model.utils import RouteSwitchModel, update_model_kwargs
from ..ragged import RaggedTensor
from .. import _ffi

__model_version__ = "2022.11.25"

model_default = {
    "name": "Megnet",
    "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 3), "name": "node_coordinates", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": [], "name": "graph_attributes", "dtype": "float32", "ragged": False}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64},
                        "graph": {"input_dim": 100, "output_dim": 64}},
    "make_distance": True, "expand_distance": True,
    "gauss_args": {"bins": 20, "distance": 4, "offset": 0.0, "sigma": 0.4},
    "meg_block_args": {"node_embed": [64, 32, 32], "edge_embed": [64, 32, 32],
                       "env_embed": [64, 32, 32], "activation": "kgcnn>softplus2"},
    "set2set_args": {"channels": 16, "T": 3, "pooling_method": "sum", "init_qstar": "0"},
    "node_ff_args": {"units": [64, 32], "activation": "kgcnn>softplus2"},
    "edge_ff_args": {"units": [64, 32], "activation": "kgcnn>softplus2"},
    "state_ff_args": {"units": [64, 32], "activation": "kgcnn>softplus2"},
    "nblocks": 3, "has_ff": True, "dropout": None, "use_set2set": True,
    "verbose": 10,
    "output_embedding": "graph",
    "output_mlp": {"use_bias": [True, True, True], "units": [32, 16, 1],
                   "activation": ["kgcnn>softplus2", "kgcnn>softplus2", "linear"]}
}

model_crystal_default = {
    "name": "Megnet",
    "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 3), "name": "node_coordinates", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": [1], "name": "charge", "dtype": "float32", "ragged": False},
               {"shape": (None, 3), "name": "edge_image", "dtype": "int64", "ragged": True},
               {"shape": (3, 3), "name": "graph_lattice", "dtype": "float32", "ragged": False}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64},
                        "graph": {"input_dim": 100, "output_dim": 64}},
    "make_distance": True, "expand_distance": True,
    "gauss_args": {"bins": 20, "distance": 4, "offset": 0.0, "sigma": 0.4},
    "meg_block_args": {"node_embed": [64, 32, 32], "edge_embed": [64, 32, 32],
                       "env_embed": [64, 32, 32], "activation": "kgcnn>softplus2"},
    "set2set_args": {"channels": 16, "T": 3, "pooling_method": "sum", "init_qstar": "0"},
    "node_ff_args": {"units": [64, 32], "activation": "kgcnn>softplus2"},
    "edge_ff_args": {"units": [64, 32], "activation": "kgcnn>softplus2"},
    "state_ff_args": {"units": [64, 32], "activation": "kgcnn>softplus2"},
    "nblocks": 3, "has_ff": True, "dropout": None, "use_set2set": True,
    "verbose": 10,
    "output_embedding": "graph",
    "output_mlp": {"use_bias": [True, True, True], "units": [32, 16, 1],
                   "activation": ["kgcnn>softplus2", "kgcnn>softplus2", "linear"]}
}


class _MegnetModel(RouteSwitchModel):
    """``Model`` with the ``use_fused_edge`` switch over all blocks."""

    switch_attr, switch_layers_attr = "use_fused_edge", "blocks"
    blocks = ()
    use_fused_edge = RouteSwitchModel.switch


@update_model_kwargs(model_default)
def make_model(inputs: list = None, input_embedding: dict = None, expand_distance: bool = None,
               make_distance: bool = None, gauss_args: dict = None, meg_block_args: dict = None,
               set2set_args: dict = None, node_ff_args: dict = None, edge_ff_args: dict = None,
               state_ff_args: dict = None, use_set2set: bool = None, nblocks: int = None, has_ff: bool = None,
               dropout: float = None, name: str = None, verbose: int = None, output_embedding: str = None,
               output_mlp: dict = None):
    r"""Build MEGNet (kgcnn/literature/Megnet.py:50-193).  Model inputs ``[node_attributes, node_coordinates |
    edge_distance, edge_indices, graph_attributes]``; output ``(batch, L)`` graph embedding.
    ``model.fused_edge_blocks`` lists which blocks fit the fused edge kernel; ``model.blocks[i].use_fused_edge`` /
    ``model.use_fused_edge`` switch it."""
    return _make(False, inputs, input_embedding, expand_distance, make_distance, gauss_args, meg_block_args, set2set_args,
                 node_ff_args, edge_ff_args, state_ff_args, use_set2set, nblocks, has_ff, dropout, name,
                 output_embedding, output_mlp)


@update_model_kwargs(model_crystal_default)
def make_crystal_model(inputs: list = None, input_embedding: dict = None, expand_distance: bool = None,
                       make_distance: bool = None, gauss_args: dict = None, meg_block_args: dict = None,
                       set2set_args: dict = None, node_ff_args: dict = None, edge_ff_args: dict = None,
                       state_ff_args: dict = None, use_set2set: bool = None, nblocks: int = None, has_ff: bool = None,
                       dropout: float = None, name: str = None, verbose: int = None, output_embedding: str = None,
                       output_mlp: dict = None):
    r"""Build MEGNet for periodic structures (kgcnn/literature/Megnet.py:222-373).  Model inputs ``[node_attributes,
    node_coordinates | edge_distance, edge_indices, state_attributes, edge_image, graph_lattice]``: ``edge_image`` ragged
    ``(batch, [M], 3)`` int64, ``graph_lattice`` dense ``(batch, 3, 3)`` with the lattice vectors in rows (what
    ``SetRangePeriodic`` takes), ``state_attributes`` dense ``(batch, F)``, or ``(batch,)`` through the embedding.  With
    ``make_distance=False`` the second input holds the distances and the last two are not read.  Output ``(batch, L)``
    graph embedding.  ``model.fused_edge_blocks`` / ``model.use_fused_edge`` as in ``make_model``."""
    if inputs is None or len(inputs) < 6:
        raise ValueError("Megnet.make_crystal_model needs six inputs (node, xyz, edge_indices, state, edge_image, "
                         "graph_lattice)")
    return _make(True, inputs, input_embedding, expand_distance, make_distance, gauss_args, meg_block_args, set2set_args,
                 node_ff_args, edge_ff_args, state_ff_args, use_set2set, nblocks, has_ff, dropout, name,
                 output_embedding, output_mlp)


def _make(crystal, inputs, input_embedding, expand_distance, make_distance, gauss_args, meg_block_args, set2set_args,
          node_ff_args, edge_ff_args, state_ff_args, use_set2set, nblocks, has_ff, dropout, name, output_embedding,
          output_mlp):
    """Both builders: the same layers in the same order; ``crystal`` adds the lattice shift of the sender positions."""
    if output_embedding != "graph":
        raise ValueError("Unsupported output embedding for mode `Megnet`.")
    if dropout is not None:
        raise NotImplementedError("dropout is not implemented: the engine has no Dropout layer")
    embed_n = OptionalInputEmbedding(**input_embedding["node"], use_embedding=len(inputs[0]["shape"]) < 2)
    embed_u = OptionalInputEmbedding(**input_embedding["graph"], use_embedding=len(inputs[3]["shape"]) < 1)
    lay_pos, lay_dist = (NodePosition(), NodeDistanceEuclidean()) if make_distance else (None, None)
    lay_shift = ShiftPeriodicLattice() if (make_distance and crystal) else None
    lay_gauss = GaussBasisLayer(**gauss_args) if expand_distance else None
    ff = [(GraphMLP(**node_ff_args), GraphMLP(**edge_ff_args), MLP(**state_ff_args))]
    blocks = []
    for i in range(nblocks):
        if has_ff and i > 0:
            ff.append((GraphMLP(**node_ff_args), GraphMLP(**edge_ff_args), MLP(**state_ff_args)))
        blocks.append(MEGnetBlock(**meg_block_args))
    adds = [(LazyAdd(), LazyAdd()) for _ in range(nblocks)]
    if use_set2set:
        dense_v, dense_e = Dense(set2set_args["channels"], activation="linear"), Dense(set2set_args["channels"],
                                                                                        activation="linear")
        read_v, read_e = PoolingSet2Set(**set2set_args), PoolingSet2Set(**set2set_args)
    else:
        dense_v = dense_e = None
        read_v, read_e = PoolingNodes(), PoolingGlobalEdges()
    out_mlp = MLP(**output_mlp)

    def forward(model_inputs, **kwargs):
        if crystal and make_distance and len(model_inputs) < 6:
            raise ValueError("Megnet (crystal) expects [node_attributes, node_coordinates, edge_indices, "
                             "state_attributes, edge_image, graph_lattice]")
        node_input, xyz_input, edi, env_input = model_inputs[:4]
        for x in model_inputs:
            # the per-graph pools read the host copy of the splits: taken once from the inputs (device-built lists,
            # SetRangePeriodic's, carry none), every derived tensor inherits it and the call sequence can be captured
            if isinstance(x, RaggedTensor):
                x.row_splits_host()
        n = embed_n(node_input)
        uenv = embed_u(env_input)
        if make_distance:
            pos1, pos2 = lay_pos([xyz_input, edi])
            if crystal:
                pos2 = lay_shift([pos2, model_inputs[4], model_inputs[5]])
            ed = lay_dist([pos1, pos2])
        else:
            ed = xyz_input
        if expand_distance:
            ed = lay_gauss(ed)
        vp, ep, up = ff[0][0](n), ff[0][1](ed), ff[0][2](uenv)
        vp2, ep2, up2 = vp, ep, up
        for i in range(nblocks):
            if has_ff and i > 0:
                vp2, ep2, up2 = ff[i][0](vp), ff[i][1](ep), ff[i][2](up)
            vp2, ep2, up2 = blocks[i]([vp2, ep2, edi, up2])
            vp = adds[i][0]([vp2, vp])          # skip connections (Megnet.py:163-165)
            ep = adds[i][1]([ep2, ep])
            up = binary_values(_ffi.MP_ADD, up2.contiguous(), up.contiguous())   # dense state: on the tape too
        if use_set2set:
            vp, ep = read_v(dense_v(vp)), read_e(dense_e(ep))
        else:
            vp, ep = read_v(vp), read_e(ep)
        flat = lambda t: t.reshape(int(t.shape[0]), -1).contiguous()    # ks.layers.Flatten
        final_vec = concat_last([flat(vp), flat(ep), up.contiguous()])
        return out_mlp(final_vec)

    # weights in construction order, so set_weights() works before a first call
    node_dim = input_embedding["node"]["output_dim"] if len(inputs[0]["shape"]) < 2 else inputs[0]["shape"][-1]
    env_dim = input_embedding["graph"]["output_dim"] if len(inputs[3]["shape"]) < 1 else inputs[3]["shape"][-1]
    edge_dim = gauss_args["bins"] if expand_distance else inputs[1]["shape"][-1]
    embed_n.ensure_built((None, None))
    embed_u.ensure_built((None,))
    last = lambda args: args["units"][-1] if isinstance(args["units"], (list, tuple)) else args["units"]
    dims = (node_dim, edge_dim, env_dim)
    block_out = (meg_block_args["node_embed"][-1], meg_block_args["edge_embed"][-1], meg_block_args["env_embed"][-1])
    layers = [embed_n, embed_u]
    k = 0
    for i in range(nblocks):
        if i == 0 or has_ff:
            trio = ff[k]
            k += 1
            trio[0].ensure_built((None, None, dims[0]))
            trio[1].ensure_built((None, None, dims[1]))
            trio[2].ensure_built((None, dims[2]))
            layers += list(trio)
            cur = (last(node_ff_args), last(edge_ff_args), last(state_ff_args))
        else:
            cur = dims
        blocks[i].ensure_built([(None, None, cur[0]), (None, None, cur[1]), (None, None, 2), (None, cur[2])])
        layers.append(blocks[i])
        dims = block_out
    if use_set2set:
        dense_v.ensure_built((None, None, dims[0]))
        dense_e.ensure_built((None, None, dims[1]))
        read_v.ensure_built((None, None, set2set_args["channels"]))
        read_e.ensure_built((None, None, set2set_args["channels"]))
        layers += [dense_v, dense_e, read_v, read_e]
        final_dim = 4 * set2set_args["channels"] + dims[2]
    else:
        final_dim = dims[0] + dims[1] + dims[2]
    out_mlp.ensure_built((None, final_dim))
    layers.append(out_mlp)
    config = {"inputs": inputs, "input_embedding": input_embedding, "make_distance": make_distance,
              "expand_distance": expand_distance, "gauss_args": gauss_args, "meg_block_args": meg_block_args,
              "set2set_args": set2set_args, "node_ff_args": node_ff_args, "edge_ff_args": edge_ff_args,
              "state_ff_args": state_ff_args, "use_set2set": use_set2set, "nblocks": nblocks, "has_ff": has_ff,
              "output_embedding": output_embedding, "output_mlp": output_mlp}
    model = _MegnetModel(name, forward, layers, config=config)
    model.__kgcnn_model_version__ = __model_version__
    model.blocks = blocks
    model.fused_edge_blocks = [bool(lay.fused_edge) for lay in blocks]
    model.auto_graph = True   # re-bound inputs replay the whole layer sequence from one HIP graph (model/utils.py)
    return model
