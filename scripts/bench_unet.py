"""Graph U-Net on 128 molecule graphs of ``synth.unet_batch`` (about 1 600 atoms, 3 500 directed bonds), the default
model (depth 4, k = 0.3, reconnect on, width 32) on feature inputs - 12 continuous node features, one positive edge
weight - with ``synth.unet_params``.  (On the embedded inputs of ``model_default`` a molecule has a handful of distinct
node rows, scores tie by coincidences of rounding and two float32 implementations may keep different nodes; continuous
features leave the ties between equal neighbour lists, which every implementation resolves alike.)

Steps (HIP events, median of --steps calls after --warmup calls):

* ``engine``: the eager forward on re-bound inputs (the input's index plan is cached on the tensors, as in every later
  call of a training or inference loop; this model is not captured into a HIP graph, its sizes are data dependent);
  engine calls and host reads (``.cpu()`` / ``.item()``) per forward;
* ``torch``: a padded dense restatement of the same network in PyTorch on the same device - ``(batch, Nmax, F)`` nodes, a
  ``(batch, Nmax, Nmax)`` adjacency, ``A @ A`` as a batched matmul, the selection by a stable sort - eager, the inputs
  padded beforehand (padding is not timed); its largest difference from the engine's output and the number of graphs
  that differ by more than 1e-5 (a graph whose scores come within rounding of each other at a cut may keep other nodes).

The parent of this model cannot run Graph U-Net, so there is no earlier time to hold these to.

Every step runs in a child process of its own under its own time limit; the first step that fails or runs out of time
ends the run (nothing more is started on the device).  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

STEPS = ["engine", "torch"]
STEP_LIMIT_S = 120
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-7


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, steps, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([_event_ms(fn) for _ in range(steps)]))


def padded_inputs(b, weights, k, depth):
    """Device tensors of the padded form: node features ``(G, Nmax, F)``, adjacency weights ``(G, Nmax, Nmax)``, node mask,
    and per level the ``(nremove, nkeep)`` of every graph (functions of the sizes)."""
    import numpy as np
    import torch
    from gcnn_keras_amd.layers.pool.topk import topk_counts
    ns, es = b["node_splits"], b["edge_splits"]
    g, sizes = len(ns) - 1, np.diff(ns)
    nmax = int(sizes.max())
    dev = weights[0].device
    x = torch.zeros((g, nmax, b["node_attributes"].shape[1]), device=dev)
    adj = torch.zeros((g, nmax, nmax), device=dev)
    mask = torch.zeros((g, nmax), dtype=torch.bool, device=dev)
    idx = torch.from_numpy(b["edge_indices"]).to(dev)
    gid_n = torch.from_numpy(np.repeat(np.arange(g), sizes)).to(dev)
    gid_e = torch.from_numpy(np.repeat(np.arange(g), np.diff(es))).to(dev)
    pos_n = torch.from_numpy(np.arange(int(ns[-1])) - np.repeat(ns[:-1], sizes)).to(dev)
    x[gid_n, pos_n] = torch.from_numpy(b["node_attributes"]).to(dev)
    mask[gid_n, pos_n] = True
    adj[gid_e, idx[:, 0], idx[:, 1]] = torch.from_numpy(b["edge_weights"][:, 0]).to(dev)
    levels, lengths = [], sizes
    for _ in range(depth):
        rem, keep = topk_counts(k, lengths)
        levels.append((torch.from_numpy(rem).to(dev), torch.from_numpy(keep).to(dev), int(keep.max()) if g else 0))
        lengths = keep
    return x, adj, mask, levels


def forward_padded(weights, x, adj, mask, levels, depth, use_reconnect=True):
    """The network of literature/Unet.py on padded dense tensors (graph output)."""
    import torch
    w = list(weights)
    w0, b0 = w.pop(0), w.pop(0)
    down = [(w.pop(0), w.pop(0), w.pop(0)) for _ in range(depth)]
    up = [(w.pop(0), w.pop(0)) for _ in range(depth)]
    wm0, bm0, wm1 = w

    def conv(h, a, m, wk, bk):
        pattern = (a != 0).to(h.dtype)
        deg = pattern.sum(-1, keepdim=True).clamp(min=1.0)
        return torch.relu(pattern @ (h @ wk + bk) / deg) * m.unsqueeze(-1)

    h = (x @ w0 + b0) * mask.unsqueeze(-1)
    saved = []
    for (wk, bk, p), (rem, keep, kmax) in zip(down, levels):
        a_in, h_in, m_in = adj, h, mask
        h = conv(h, adj, mask, wk, bk)
        if use_reconnect:
            adj = adj @ adj
            adj = torch.where(adj > EPS, adj, torch.zeros_like(adj))
        s = (h * p / torch.sqrt((p * p).sum())).sum(-1)
        order = torch.argsort(torch.where(mask, s, torch.full_like(s, float("inf"))), dim=1, stable=True)
        slot = rem.unsqueeze(1) + torch.arange(kmax, device=h.device).unsqueeze(0)
        new_mask = torch.arange(kmax, device=h.device).unsqueeze(0) < keep.unsqueeze(1)
        sel = torch.gather(order, 1, slot.clamp(max=order.shape[1] - 1))
        gate = torch.sigmoid(torch.gather(s, 1, sel)).unsqueeze(-1)
        hp = torch.gather(h, 1, sel.unsqueeze(-1).expand(-1, -1, h.shape[2])) * gate * new_mask.unsqueeze(-1)
        ap = torch.gather(torch.gather(adj, 1, sel.unsqueeze(-1).expand(-1, -1, adj.shape[2])), 2,
                          sel.unsqueeze(1).expand(-1, kmax, -1))
        ap = ap * (new_mask.unsqueeze(1) & new_mask.unsqueeze(2))
        saved.append((h_in, a_in, m_in, sel, new_mask))
        h, adj, mask = hp, ap, new_mask
    for (wk, bk), (h_old, a_old, m_old, sel, new_mask) in zip(up, reversed(saved)):
        back = torch.zeros_like(h_old)
        back.scatter_add_(1, sel.unsqueeze(-1).expand(-1, -1, h.shape[2]), h * new_mask.unsqueeze(-1))
        h = conv(back + h_old, a_old, m_old, wk, bk)
        mask = m_old
    pooled = h.sum(1) / mask.sum(1, keepdim=True).clamp(min=1).to(h.dtype)
    return torch.sigmoid(torch.relu(pooled @ wm0 + bm0) @ wm1)


def run_step(step, args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from gcnn_keras_amd import _ffi, synth
    from gcnn_keras_amd.literature import Unet
    from gcnn_keras_amd.ragged import RaggedTensor
    if not torch.cuda.is_available():
        raise SystemExit("bench_unet.py needs an MI355X: no device, no timing")
    b = synth.unet_batch(args.graphs)
    ns, es = b["node_splits"], b["edge_splits"]
    rag = lambda v, s: RaggedTensor.from_numpy(np.ascontiguousarray(v), s)
    res = {"graphs": args.graphs, "atoms": int(ns[-1]), "edges": int(es[-1]), "largest": int(np.diff(ns).max())}
    inputs = [{"shape": (None, int(b["node_attributes"].shape[1])), "name": "node_attributes", "dtype": "float32",
               "ragged": True},
              {"shape": (None, 1), "name": "edge_attributes", "dtype": "float32", "ragged": True},
              {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}]
    m = Unet.make_model(inputs=inputs, verbose=30)
    params = synth.unet_params(m)
    m.set_weights(list(params.values()))
    depth, k = m.config["depth"], m.config["top_k_args"]["k"]
    x = [rag(b["node_attributes"], ns), rag(b["edge_weights"], es), rag(b["edge_indices"], es)]
    with torch.no_grad():
        if step == "engine":
            m(x)
            reads = [0]
            cpu, item = torch.Tensor.cpu, torch.Tensor.item

            def counting(fn):
                def wrapped(self, *a, **kw):
                    reads[0] += 1 if self.is_cuda else 0
                    return fn(self, *a, **kw)
                return wrapped

            torch.Tensor.cpu, torch.Tensor.item = counting(cpu), counting(item)
            before = _ffi.launch_count()
            m(x)
            res["launches"], res["host_reads"] = _ffi.launch_count() - before, reads[0]
            torch.Tensor.cpu, torch.Tensor.item = cpu, item
            res["eager_ms"] = timed(lambda: m(x), args.steps, args.warmup)
            res["route"] = m.last_route
        else:
            weights = [torch.from_numpy(v).cuda() for v in params.values()]
            xp, adj, mask, levels = padded_inputs(b, weights, k, depth)
            fn = lambda: forward_padded(weights, xp, adj, mask, levels, depth)
            res["torch_padded_eager_ms"] = timed(fn, args.steps, args.warmup)
            got, want = m(x), fn()
            diff = (got - want[:got.shape[0]]).abs()
            res["max_abs_diff_engine_vs_torch"] = float(diff.max())
            res["graphs_differing_by_more_than_1e-5"] = int((diff > 1e-5).sum())
            res["max_abs_output"] = float(want.abs().max())
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=128)
    ap.add_argument("--step", choices=STEPS, default=None, help="run this one step in this process")
    args = ap.parse_args()
    if args.step is not None:
        run_step(args.step, args)
        return
    res = {"steps": args.steps, "warmup": args.warmup}
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", step,
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--graphs", str(args.graphs)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if done.returncode != 0:
            res["failed"] = {"step": step, "returncode": done.returncode}
            print(json.dumps(res))
            raise SystemExit(1)
        res[step] = json.loads(done.stdout.strip().splitlines()[-1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
