#!/usr/bin/env python3
"""Shape-edge fixtures from the CPU oracle in float64 (no reference import; run from the repository root):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_edge_golden.py [case ...]

The host schedule of libmatgcn picks kernels by N and B and by the configuration ("Shape edges"); every case
below is the smallest shape on one side of such a rule.  The cases are built exactly as
test_backward_on_synthetic_shapes_outside_the_golden_set builds its own (synthetic data feature of seed 3, the host graph
prep, closed-form parameters of seed 3; by default multi / unidirection / cheb_order 2, two layers, two input channels,
embed_dim_node 20, 24 -> 6 steps, no initial state), run through oracle.forward(faithful=False) in float64 and, for the
gradient cases, through (y * d_out).sum().backward() with d_out = default_rng(9).standard_normal.  A case may carry a
configuration of its own (the keys of DEFAULTS below; edge_index.json holds the whole configuration of every case and
default_config = whether it is the default one): cheb, adjtype, adpadj, layers, ext (0 / 1 / 8 / 13 input channels next to the flow, as test_backward_gpu.py maps
them to add_time_in_day / add_day_in_week / load_dynamic), end_dim, out, embed, h0 (a seeded (N, H) initial state,
0.1 * default_rng(11).standard_normal, handed to oracle.forward(h0=) as a leaf; its gradient is stored as
grad.__d_h0__ - what the HIP path's d_h0 (L, B, N, H) sums to over layers and batch) and sub (the stride of the
subsampled gradients).  Stored (data only):

  edge_<case>.npz       pred64 (float64, whole), x_checksum / param_checksum / static_sums as synth4096_out24.npz has
                        them, gap32_pred = the oracle's own fp32 run against its fp64 run on the same input
                        (max-normalised)
  edge_grad_<case>.npz  the same three checksums, gap32_grad (worst tensor of the fp32 oracle's autograd against the fp64
                        one) and the gradients in the layout of grad_*.npz: `grad.<name>` whole up to 20000 elements, else
                        `gsub.<name>` (every `sub`-th element of the flattened tensor) + `gsum.<name>` [sum, sum |.|].
                        Gradients are stored as float32 (as grad_*.npz are): 6e-8 relative, 1/1600 of the tolerance they
                        are compared with; the sums stay float64.

The prediction and the gradients live in two files so that every file stays below 1 MiB (pred64 of B = 65, N = 257 is
0.8 MB by itself).  SUB = 61 (prime) keeps the largest gradient file of the default configuration near 0.65 MB; the
cases whose support stack or embedding multiplies the pooled weights take a larger prime, so that every file stays
below 1 MiB and the configuration cases together below 8 MB.  The files are written with fixed zip time stamps: a second
run leaves every byte as it is.

Admission rule of every case, added or moved: the oracle's own fp32-vs-fp64 gap is at most GAP_MAX = 5e-6 on the
prediction and on the worst gradient tensor (1/20 of the 1e-4 the tests use) - a case that misses is not written.  The
Chebyshev recursion is ill-conditioned in fp32 itself on some supports (cheb_order 4 on od / unidirection and cheb_order
5 on dist / none at N = 65 miss by two orders of magnitude): such a case would test the number format, not the kernels.
"""
import io
import json
import os
import sys
import time
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from multistgraph_amd import graph_prep, synthetic as syn  # noqa: E402
from multistgraph_amd.ops import HotPath  # noqa: E402
from oracle import matgcn_oracle as orc  # noqa: E402

SUB = 61
SEED = 3
OUT = 6
WHOLE = 20000
GAP_MAX = 5e-6
D_H0 = HotPath.D_H0     # key of the initial-state gradient, as HotPath.backward names it

DEFAULTS = dict(cheb=2, adjtype="multi", adpadj="unidirection", layers=2, ext=1, end_dim=1, out=OUT, embed=20, h0=False,
                sub=SUB)

# name, N, B, gradient fixture[, configuration]
CASES = [
    ("edge_n48_b3", 48, 3, True),
    ("edge_n64_b17", 64, 17, True),
    ("edge_n65_b16", 65, 16, True),
    ("edge_n256_b33", 256, 33, True),
    ("edge_n257_b33", 257, 33, True),
    ("edge_n257_b65", 257, 65, True),
    ("edge_n256_b65", 256, 65, False),
    ("edge_n263_b8", 263, 8, False),
    ("edge_n1024_b2", 1024, 2, False),
    ("edge_n1039_b3", 1039, 3, True),
    ("edge_n1039_b2", 1039, 2, False),
    ("edge_n21_b129", 21, 129, False),
    # configuration-dependent kernel choices past one tile (test_shape_edges.py has the rule of each)
    ("edge_c3_n65_b5", 65, 5, True, dict(cheb=3, sub=97)),
    ("edge_c3bi_n257_b3", 257, 3, True, dict(cheb=3, adpadj="bidirection", h0=True, sub=97)),
    ("edge_c3none_n80_b17", 80, 17, True, dict(cheb=3, adpadj="none", sub=97)),
    ("edge_c4_n65_b3", 65, 3, True, dict(cheb=4, sub=127)),
    ("edge_c1_n65_b17_l3", 65, 17, True, dict(cheb=1, layers=3)),
    ("edge_oduni_n65_b3", 65, 3, True, dict(adjtype="od")),
    ("edge_dist_n65_b33_l1", 65, 33, True, dict(adjtype="dist", adpadj="none", layers=1)),
    ("edge_ident_c3_n65_b5", 65, 5, True, dict(cheb=3, adjtype="identity", adpadj="none")),
    ("edge_ext13_n65_b7", 65, 7, True, dict(ext=13)),
    ("edge_ext8_n48_b17", 48, 17, True, dict(ext=8)),
    ("edge_ext0_n65_b16", 65, 16, True, dict(ext=0)),
    ("edge_od2_out24_n65_b3", 65, 3, True, dict(end_dim=2, out=24)),
    ("edge_l4_n48_b3", 48, 3, True, dict(layers=4, h0=True, sub=127)),
    ("edge_emb8_n65_b3", 65, 3, True, dict(embed=8)),
    ("edge_emb40_n65_b3", 65, 3, True, dict(embed=40, sub=97)),
]


def case_table():
    """[(name, N, B, gradient fixture, the case's own keys, its full configuration)]"""
    rows = []
    for row in CASES:
        own = dict(row[4]) if len(row) > 4 else {}
        assert set(own) <= set(DEFAULTS), own
        rows.append(row[:4] + (own, dict(DEFAULTS, **own)))
    return rows


def oracle_cfg(k):
    ext = k["ext"]
    return dict(adjtype=k["adjtype"], adpadj=k["adpadj"], cheb_order=k["cheb"], num_layers=k["layers"], rnn_units=64,
                len_closeness=48, len_period=24, len_trend=24, output_window=k["out"], input_window=24,
                add_time_in_day=ext > 0, add_day_in_week=ext in (8, 13), load_dynamic=ext == 13, start_dim=0,
                end_dim=k["end_dim"])


def use_static(k):
    """the reference keeps the static supports next to the adaptive one in 'multi' mode only (MultiATGCN.py:90-93)"""
    return k["adpadj"] == "none" or k["adjtype"] == "multi"


def build_case(n, b, k):
    """inputs of one case: data feature, static supports (K, N, N) float32, parameters, x, initial state - all numpy"""
    od, ext = k["end_dim"], k["ext"]
    df = syn.make_data_feature(n, SEED, "DC", ext_dim=ext)
    mats = np.stack(graph_prep.build_static_supports(df["adj_mx"], df["coordinate"], None, k["adjtype"]), 0)
    shapes = syn.param_shapes(n, out_steps=k["out"], feat_in=od + ext, out_dim=od,
                              k_total=syn.k_total_for(k["adjtype"], k["adpadj"], k["cheb"]),
                              layers=k["layers"], embed_dim_node=k["embed"], len_ts=4)
    state = syn.closed_form_state(shapes, SEED)
    x, _ = syn.make_batch_arrays(b, n, k["out"], SEED, feat=od + ext)
    if od > 1:   # channels [flow 0 .. flow od-1 | time of day]
        x = np.ascontiguousarray(np.concatenate([x[..., :1], x[..., 2:], x[..., 1:2]], -1))
    h0 = (0.1 * np.random.default_rng(11).standard_normal((n, 64))).astype(np.float32) if k["h0"] else None
    return df, mats, state, x, h0


def checksums(mats, state, x):
    m64 = mats.astype(np.float64)
    return {"x_checksum": np.float64(x.astype(np.float64).sum()),
            "param_checksum": np.float64(sum(float(np.abs(v.astype(np.float64)).sum()) for v in state.values())),
            "static_sums": np.stack([m64.sum((1, 2)), np.abs(m64).sum((1, 2))], 1)}


def d_out_for(n, b, k):
    return np.random.default_rng(9).standard_normal((b, k["out"], n, k["end_dim"])).astype(np.float32)


def max_norm(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def run(mats, state, x, d_out, dtype, k, h0=None):
    """prediction and (d_out given) every parameter gradient of the oracle in `dtype`, as float64 numpy"""
    p = {name: torch.tensor(v, dtype=dtype, requires_grad=d_out is not None) for name, v in state.items()}
    st = [torch.from_numpy(m).to(dtype) for m in mats] if use_static(k) else []
    init = None if h0 is None else torch.tensor(h0, dtype=dtype, requires_grad=d_out is not None)
    with torch.set_grad_enabled(d_out is not None):
        y = orc.forward(torch.tensor(x, dtype=dtype), p, st, oracle_cfg(k), faithful=False, h0=init)
        assert y.dtype == dtype
        if d_out is None:
            return y.numpy().astype(np.float64), None
        (y * torch.tensor(d_out, dtype=dtype)).sum().backward()
    grads = {name: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)).astype(np.float64)
             for name, v in p.items()}
    if init is not None:
        grads[D_H0] = init.grad.numpy().astype(np.float64)
    return y.detach().numpy().astype(np.float64), grads


def save(path, arrays):
    """np.savez_compressed with fixed member time stamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    only = set(sys.argv[1:])
    for name, n, b, with_grad, own, k in case_table():
        if only and name not in only:
            continue
        t0 = time.time()
        df, mats, state, x, h0 = build_case(n, b, k)
        sums = checksums(mats, state, x)
        d_out = d_out_for(n, b, k) if with_grad else None
        y64, g64 = run(mats, state, x, d_out, torch.float64, k, h0)
        y32, g32 = run(mats, state, x, d_out, torch.float32, k, h0)
        gap_pred = max_norm(y32, y64)
        line = "%-22s N %4d B %3d  %5.0f s  gap32_pred %.2e" % (name, n, b, time.time() - t0, gap_pred)
        # the admission rule of every case, added or moved: it must test the kernels, not fp32 itself
        assert gap_pred <= GAP_MAX, "%s: gap32_pred %.2e > %.0e - not written" % (name, gap_pred, GAP_MAX)
        if with_grad:
            gaps = {key: max_norm(g32[key], g64[key]) for key in g64 if np.abs(g64[key]).max() > 0.0}
            worst = max(gaps, key=gaps.get)
            line += "  gap32_grad %.2e (%s)" % (gaps[worst], worst)
            assert gaps[worst] <= GAP_MAX, "%s: gap32_grad %.2e (%s) > %.0e - not written" % (
                name, gaps[worst], worst, GAP_MAX)
            out = dict(sums, sub=np.int64(k["sub"]), gap32_grad=np.float64(gaps[worst]))
            for key, g in g64.items():
                if g.size <= WHOLE:
                    out["grad." + key] = g.astype(np.float32)
                else:
                    out["gsub." + key] = g.reshape(-1)[::k["sub"]].astype(np.float32)
                    out["gsum." + key] = np.array([g.sum(), np.abs(g).sum()])
            save(os.path.join(HERE, "edge_grad_%s.npz" % name[5:]), out)
        save(os.path.join(HERE, name + ".npz"), dict(sums, pred64=y64, gap32_pred=np.float64(gap_pred)))
        print(line, flush=True)
    if not only:
        index = {}
        for name, n, b, g, own, k in case_table():
            # the whole configuration of every case, so that nobody who reads the index needs a copy of DEFAULTS;
            # default_config: the case differs from the others of its kind by shape alone (`sub` is no configuration)
            index[name] = dict(k, name=name, nodes=n, batch=b, feat=k["end_dim"] + k["ext"], seed=SEED, city="DC",
                               grad=bool(g), default_config=not (set(own) - {"sub"}))
        with open(os.path.join(HERE, "edge_index.json"), "w") as fh:
            json.dump(index, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
