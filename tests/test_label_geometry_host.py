"""The label geometry every label-reading entry point refuses (include/matgcn.h, "the label contract"): one table of
refused (batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, label_start), applied to all twelve entry points with
the status each returns written out.  The strict rule (y_steps >= out_steps, windows or series) holds for the two
matgcn_masked_mae, the two matgcn_loss, the two matgcn_metric_sums and the two matgcn_region_loss entry points; the series
rule (y_steps >= 1 and y_feat >= 1, y_steps >= out_steps for windows only) for matgcn_mc_scores, matgcn_mc_scores_nodes,
matgcn_mc_conformity and matgcn_group_label_sums.  Every call is refused before its launch, so pointers that nothing
dereferences do; a case an entry point would accept is left out of its column (it would launch).  No GPU."""
import ctypes as C

import pytest

BAD_ARG = -2
__ = None                  # not applied: the entry point accepts this geometry
PTR = C.c_void_p(4096)     # a non-NULL, 8-byte aligned pointer nothing dereferences
NAN = float("nan")

ENTRIES = ("matgcn_masked_mae", "matgcn_masked_mae_grad", "matgcn_loss", "matgcn_loss_grad", "matgcn_metric_sums",
           "matgcn_metric_sums_nodes", "matgcn_region_loss", "matgcn_region_loss_grad",
           "matgcn_mc_scores", "matgcn_mc_scores_nodes", "matgcn_mc_conformity", "matgcn_group_label_sums")
STRICT, SERIES_RULE = ENTRIES[:8], ENTRIES[8:]

# an accepted geometry: every case changes the fields it names
BASE = dict(batch=2, out_steps=3, nodes=5, out_dim=2, y_steps=3, y_feat=3, y_start=1, series=False)

# case, changed fields, status per entry point in the order of ENTRIES.  A case an entry point would accept cannot be here, so
# some clauses are pinned by one case only: windows_without_steps is already refused as windows shorter than out_steps and
# the two *no_label_channels cases as y_start + out_dim > y_feat; series_without_steps alone reaches the series rule's
# y_steps >= 1 (a series needs no out_steps rows there), and series_shorter_than_out_steps alone tells the two rules apart.
#                                                                          mae  mae_g loss loss_g sums sums_n reg  reg_g | mc   mc_n conf g_lab
REFUSED = [
    ("windows_one_step_short", dict(y_steps=2),                           (-2,  -2,   -2,  -2,    -2,  -2,    -2,  -2,     -2,  -2,  -2,  -2)),
    ("series_shorter_than_out_steps", dict(y_steps=2, series=True),       (-2,  -2,   -2,  -2,    -2,  -2,    -2,  -2,     __,  __,  __,  __)),
    ("windows_without_steps", dict(y_steps=0),                            (-2,  -2,   -2,  -2,    -2,  -2,    -2,  -2,     -2,  -2,  -2,  -2)),
    ("series_without_steps", dict(y_steps=0, series=True),                (-2,  -2,   -2,  -2,    -2,  -2,    -2,  -2,     -2,  -2,  -2,  -2)),
    ("no_label_channels", dict(y_feat=0, y_start=0),                      (-2,  -2,   -2,  -2,    -2,  -2,    -2,  -2,     -2,  -2,  -2,  -2)),
    ("series_no_label_channels", dict(y_feat=0, y_start=0, series=True),  (-2,  -2,   -2,  -2,    -2,  -2,    -2,  -2,     -2,  -2,  -2,  -2)),
    ("negative_first_channel", dict(y_start=-1),                          (-2,  -2,   -2,  -2,    -2,  -2,    -2,  -2,     -2,  -2,  -2,  -2)),
    ("one_channel_past_the_end", dict(y_start=2),                         (-2,  -2,   -2,  -2,    -2,  -2,    -2,  -2,     -2,  -2,  -2,  -2)),
    ("series_one_channel_past_the_end", dict(y_start=2, series=True),     (-2,  -2,   -2,  -2,    -2,  -2,    -2,  -2,     -2,  -2,  -2,  -2)),
    ("no_nodes", dict(nodes=0),                                           (-2,  -2,   -2,  -2,    -2,  -2,    -2,  -2,     -2,  -2,  -2,  -2)),
    ("no_channels", dict(out_dim=0),                                      (-2,  -2,   -2,  -2,    -2,  -2,    -2,  -2,     -2,  -2,  -2,  -2)),
    ("no_horizons", dict(out_steps=0),                                    (-2,  -2,   -2,  -2,    -2,  -2,    -2,  -2,     -2,  -2,  -2,  -2)),
    ("horizons_past_the_cap", dict(out_steps=65, y_steps=65),             (-2,  -2,   -2,  -2,    -2,  -2,    -2,  -2,     __,  -2,  -2,  __)),
]


def _lib():
    from multistgraph_amd import _lib
    return _lib


def _groups(keep):
    """a valid map of three groups over the five nodes: host offsets real, device arrays never read"""
    g = _lib().Groups()
    host = (C.c_int32 * 4)(0, 2, 2, 6)
    keep.append(host)
    g.ptr, g.ptr_dev, g.node, g.weight = C.cast(host, C.POINTER(C.c_int32)), PTR, PTR, None
    g.n_groups, g.n_members = 3, 6
    return g


def _by_node(keep):
    g = _lib().Groups()
    host = (C.c_int32 * 6)(0, 1, 2, 4, 5, 6)
    keep.append(host)
    g.ptr, g.ptr_dev, g.node, g.weight = C.cast(host, C.POINTER(C.c_int32)), PTR, PTR, None
    g.n_groups, g.n_members = 5, 6
    return g


def _call(lib, entry, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, series):
    """the entry point on this geometry; everything else about the call is valid"""
    keep = []
    L = _lib()
    geometry = (batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start)
    labels = (PTR, PTR if series else None)
    desc = L.LossDesc(L.LOSS_MSE, 0.0, 1.0, NAN, 1e-4, 0.0)
    scale = L.MetricScale(None, None, 0, None, None, NAN, NAN, -1.0)
    probs = (C.c_float * 3)(0.05, 0.5, 0.95)
    big = 1 << 40
    fn = getattr(lib, entry)
    if entry == "matgcn_masked_mae":
        return fn(PTR, *labels, *geometry, 0.0, 1.0, NAN, 1e-4, PTR, PTR, None)
    if entry == "matgcn_masked_mae_grad":
        return fn(PTR, *labels, *geometry, 0.0, 1.0, NAN, 1e-4, PTR, PTR, PTR, None)
    if entry == "matgcn_loss":
        return fn(PTR, *labels, *geometry, C.byref(desc), PTR, big, PTR, None)
    if entry == "matgcn_loss_grad":
        return fn(PTR, *labels, *geometry, C.byref(desc), PTR, big, PTR, PTR, None)
    if entry == "matgcn_metric_sums":
        return fn(PTR, *labels, *geometry, C.byref(scale), PTR, PTR, 0, None)
    if entry == "matgcn_metric_sums_nodes":
        return fn(PTR, *labels, *geometry, C.byref(scale), PTR, big, PTR, 0, None)
    if entry == "matgcn_region_loss":
        return fn(PTR, *labels, *geometry, C.byref(desc), C.byref(_groups(keep)), PTR, big, PTR, None)
    if entry == "matgcn_region_loss_grad":
        return fn(PTR, *labels, *geometry, C.byref(desc), C.byref(_groups(keep)), C.byref(_by_node(keep)), PTR, big, PTR,
                  None, PTR, None)
    if entry == "matgcn_mc_scores":
        return fn(PTR, 8, *labels, *geometry, 0.0, 1.0, NAN, 1e-4, probs, 3, PTR, big, PTR, 0, None)
    if entry == "matgcn_mc_scores_nodes":
        return fn(PTR, 8, *labels, *geometry, C.byref(scale), NAN, probs, 3, PTR, big, PTR, 0, None)
    if entry == "matgcn_mc_conformity":
        return fn(PTR, 8, *labels, *geometry, C.byref(scale), NAN, probs, 3, PTR, None)
    assert entry == "matgcn_group_label_sums"
    return fn(*labels, *geometry, C.byref(scale), C.byref(_groups(keep)), PTR, None)


def test_the_table_names_every_label_reading_entry_point():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "matgcn.h")).read()
    # an entry point reads labels where it takes a label_start next to y
    declared = re.findall(r"int (matgcn_\w+)\(const float\* \w+,(?:[^;)]*?)const int32_t\* label_start,", header)
    assert sorted(declared) == sorted(ENTRIES)
    assert len(ENTRIES) == 12 and all(len(row[2]) == 12 for row in REFUSED)


def test_the_rule_columns_are_what_the_docstring_says():
    """the table against the module docstring, no library call: a blank may stand only where a rule accepts the case.  A series shorter than out_steps is refused by the strict eight alone; the cap of 64 horizons is not
    matgcn_mc_scores' or matgcn_group_label_sums'; every other case is every entry point's"""
    rows = {name: dict(zip(ENTRIES, status)) for name, _, status in REFUSED}
    assert [e for e in ENTRIES if rows["series_shorter_than_out_steps"][e] is not None] == list(STRICT)
    assert [e for e in ENTRIES if rows["horizons_past_the_cap"][e] is None] == ["matgcn_mc_scores",
                                                                                 "matgcn_group_label_sums"]
    for name, row in rows.items():
        if name not in ("series_shorter_than_out_steps", "horizons_past_the_cap"):
            assert None not in row.values(), name


@pytest.mark.parametrize("entry", ENTRIES)
def test_refused_geometry(lib_built, entry):
    lib = _lib().load()
    col = ENTRIES.index(entry)
    applied = 0
    for name, fields, status in REFUSED:
        if status[col] is None:
            continue
        assert status[col] != 0                                     # nothing here may launch
        assert _call(lib, entry, **dict(BASE, **fields)) == status[col], (entry, name)
        applied += 1
    assert applied >= 9
