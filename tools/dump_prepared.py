"""Dump what matgcn_prepare writes, block by block, so that two builds of the library can be compared bit for bit.

    python tools/dump_prepared.py --nodes 403 --batch 64 --out a.npz      # with build A
    python tools/dump_prepared.py --nodes 403 --batch 64 --out b.npz      # with build B
    python tools/dump_prepared.py --compare a.npz b.npz

The model is the headline configuration (multi / unidirection, cheb_order 2, two layers) on the synthetic graph of
--nodes nodes with closed-form parameters, so both runs see the same inputs.  `prepared` is zeroed first (the gaps
between its blocks are written by nobody), then prepared and joined.  Offsets: St from matgcn_supports_layout, Wg_l and
Wu_l from matgcn_weights_layout; the blocks between them follow in the order of DESIGN.md section 3, each rounded up to
64 floats - per layer Wg, Wu, (Wx, Bx from layer 1 on), Rg, Ru, then Head, and StT as the last block.  The staging
matrices plainA/B/C behind St are prepare-internal scratch and are left out.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rup(v, m=64):
    return (v + m - 1) // m * m


def dump(nodes, batch, out):
    import torch
    from multistgraph_amd import graph_prep, synthetic as syn
    from multistgraph_amd.ops import HotPath, diagonal_mask, spec_from_config
    dev = torch.device("cuda:0")
    df = syn.make_data_feature(nodes, 7, "BM" if nodes == 403 else "DC", ext_dim=1)
    mats = np.stack(graph_prep.build_static_supports(df["adj_mx"], df["coordinate"], None, "multi"), 0)
    state = syn.closed_form_state(syn.param_shapes(nodes, out_steps=3, feat_in=2,
                                                   k_total=syn.k_total_for("multi", "unidirection", 2)), 7)
    cfg = dict(input_window=24, output_window=3, add_time_in_day=True, add_day_in_week=False, load_dynamic=False,
               adjtype="multi", adpadj="unidirection", cheb_order=2, embed_dim_node=20, embed_dim_adj=20, rnn_units=64,
               num_layers=2, device=torch.device("cpu"), batch_size=batch, start_dim=0, end_dim=1)
    st = torch.from_numpy(mats)
    spec = spec_from_config(cfg, df, nodes, min(nodes, 20), st.shape[0], diagonal_mask(st))
    hp = HotPath(spec, batch, dev)
    hp.bind({k: torch.from_numpy(v).to(dev) for k, v in state.items()}, st.to(dev))
    hp.prepared.zero_()
    torch.cuda.synchronize()
    hp.prepare()
    hp.prepare_join()
    torch.cuda.synchronize()
    prep = hp.prepared.cpu().numpy()
    lay = (C.c_int64 * 4)()
    assert hp.lib.matgcn_supports_layout(C.byref(hp.dims), lay) == 0
    o_st, mp, np_, ks = (int(v) for v in lay)
    blocks = {"St": (o_st, np_ * mp)}
    layers, h, c0 = spec.layers, 64, spec.feat_in
    at = None
    for l in range(layers):
        cpad = rup(c0 if l == 0 else h, 16)
        for part, name in ((0, "Wg"), (1, "Wu")):
            assert hp.lib.matgcn_weights_layout(C.byref(hp.dims), l, part, lay) == 0
            ofs, stride = int(lay[0]), int(lay[1])
            assert at is None or at == ofs, (name, l, at, ofs)
            blocks["%s%d" % (name, l)] = (ofs, nodes * stride)
            at = ofs + rup(nodes * stride)
        if l > 0:
            wx = (ks + 1) * h * 192
            blocks["Wx%d" % l] = (at, nodes * wx)
            at += rup(nodes * wx)
            blocks["Bx%d" % l] = (at, nodes * 192)
            at += rup(nodes * 192)
        blocks["Rg%d" % l] = (at, (cpad + h) * 128)
        at += rup((cpad + h) * 128)
        blocks["Ru%d" % l] = (at, (cpad + h) * 64)
        at += rup((cpad + h) * 64)
    head_t = 1 if spec.fnn_off else spec.in_steps
    ntc = (spec.out_window * spec.out_dim + 31) // 32
    blocks["Head"] = (at, head_t * h * 32 * ntc)
    at += rup(head_t * h * 32 * ntc)
    mt = rup(ks * nodes)
    blocks["StT"] = (at, np_ * mt)
    assert at + rup(np_ * mt) == prep.size, (at, np_ * mt, prep.size)      # StT is the last block
    np.savez(out, **{k: prep[o:o + n] for k, (o, n) in blocks.items()})
    print("wrote %s: %s" % (out, ", ".join("%s[%d]" % (k, n) for k, (o, n) in blocks.items())))


def compare(a, b):
    da, db = np.load(a), np.load(b)
    bad = sorted(set(da.files) ^ set(db.files))
    for k in da.files:
        if k in db.files:
            same = da[k].shape == db[k].shape and np.array_equal(da[k].view(np.uint32), db[k].view(np.uint32))
            print("%-6s %10d floats  %s" % (k, da[k].size, "equal" if same else "DIFFERENT"))
            if not same:
                bad.append(k)
    print("bit-identical" if not bad else "differences in: %s" % ", ".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=403)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default="prepared.npz")
    ap.add_argument("--compare", nargs=2, metavar="NPZ")
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else dump(args.nodes, args.batch, args.out))
