"""The generator behind the device-side dropout, on the host: known-answer vectors of Philox4x32-10, the threshold rule,
the keep rate of the reference mask, and the library surface (symbols, binding, config key).  No GPU."""
import math
import os

import numpy as np
import pytest

import philox_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("matgcn_dropout_mask", "matgcn_forward_train_seeded", "matgcn_backward_seeded", "matgcn_forward_mc")

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_known_answer_vectors(counter, key, want):
    got = R.philox4x32_10(np.array(counter, dtype=np.uint64), key)
    assert " ".join("%08x" % int(w) for w in got) == want
    # the vectorised form gives the same words
    many = R.philox4x32_10(np.array([counter, counter], dtype=np.uint64), key)
    assert np.array_equal(many[0], got) and np.array_equal(many[1], got)


def test_threshold_and_scale():
    assert R.threshold(0.1) == 429496736 == 0x199999A0
    assert R.threshold(0.0) == 0
    assert R.threshold(0.5) == 2 ** 31
    assert R.keep_scale(0.5) == np.float32(2.0) and R.keep_scale(0.0) == np.float32(1.0)
    assert R.keep_scale(0.1) == np.float32(1.0 / (1.0 - float(np.float32(0.1))))


@pytest.mark.parametrize("shape", [(16, 24, 65), (3, 24, 48), (129, 1, 21)])
def test_keep_rate_of_the_reference_mask(shape):
    """seed 1234, offset 0, p = 0.1: the keep fraction lies within 4 sigma of 0.9, sigma = sqrt(0.09 / n)"""
    keep = R.keep_bits(*shape, seed=1234, offset=0, p=0.1)
    n = keep.size
    dev = (keep.mean() - 0.9) / math.sqrt(0.09 / n)
    print("%s: keep fraction %.6f, %.2f sigma" % (shape, keep.mean(), dev))
    assert abs(dev) <= 4.0
    m = R.mask(*shape, seed=1234, offset=0, p=0.1)
    assert m.dtype == np.float32 and set(np.unique(m)) == {np.float32(0.0), R.keep_scale(0.1)}


def test_offsets_and_seeds_give_other_masks():
    a = R.keep_bits(3, 24, 48, 1234, 0, 0.1)
    assert not np.array_equal(a, R.keep_bits(3, 24, 48, 1234, 1, 0.1))
    assert not np.array_equal(a, R.keep_bits(3, 24, 48, 1234, 2 ** 32, 0.1))      # the high word of the offset counts
    assert not np.array_equal(a, R.keep_bits(3, 24, 48, 1234 + 2 ** 32, 0, 0.1))  # and of the seed
    assert np.array_equal(a, R.keep_bits(3, 24, 48, 1234, 0, 0.1))
    assert R.keep_bits(3, 24, 48, 1234, 0, 0.0).all()


def test_library_exports_and_binding(lib_built):
    """the four new functions are exported by libmatgcn.so, declared in the header and bound by _lib.py with the struct
    they take; ABI stays 12"""
    import ctypes as C
    from multistgraph_amd import _lib
    with open(os.path.join(ROOT, "include", "matgcn.h")) as fh:
        header = fh.read()
    lib = _lib.load()
    for name in NEW_FUNCTIONS:
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert "int %s(" % name in header, name
    assert "typedef struct matgcn_dropout" in header and "#define MATGCN_MAX_MC_SAMPLES 1024" in header
    assert "#define MATGCN_ABI_VERSION 12" in header and lib.matgcn_abi_version() == 12
    assert [f[0] for f in _lib.Dropout._fields_] == ["seed", "offset", "p"]
    assert C.sizeof(_lib.Dropout) == 24 and _lib.MAX_MC_SAMPLES == 1024
    from multistgraph_amd.ops import HotPath
    for method in ("dropout_mask", "forward_mc"):
        assert callable(getattr(HotPath, method))


def test_descriptor_is_validated_on_the_host(lib_built):
    """0 <= p < 1, anything else is MATGCN_ERR_BAD_ARG - checked before any launch, so this needs no GPU; a null mask
    pointer is MATGCN_ERR_NULL"""
    import ctypes as C
    from helpers import Case
    from multistgraph_amd import _lib
    from multistgraph_amd.ops import spec_from_config
    c = Case("tiny_multi_uni_c2")
    dims = spec_from_config(c.config(), c.data_feature, c.n, min(c.n, 20), 0, 0).dims(c.b)
    lib = _lib.load()
    for p in (1.0, -0.1, 1.5, float("nan")):
        d = _lib.Dropout(1, 0, p)
        assert lib.matgcn_dropout_mask(C.byref(dims), C.byref(d), C.c_void_p(16), None) == -2, p
    assert lib.matgcn_dropout_mask(C.byref(dims), C.byref(_lib.Dropout(1, 0, 0.1)), None, None) == -1


def test_hip_dropout_key_is_validated():
    import torch
    from helpers import Case
    from multistgraph_amd.model import MultiATGCN
    c = Case("tiny_multi_uni_c2")
    torch.manual_seed(0)
    ref = MultiATGCN(c.config(), c.data_feature)
    assert ref.hip_dropout == "torch"
    torch.manual_seed(0)
    m = MultiATGCN(dict(c.config(), hip_dropout="device"), c.data_feature)
    assert m.hip_dropout == "device"
    sd, rd = m.state_dict(), ref.state_dict()
    assert list(sd) == list(rd) and all(torch.equal(sd[k], rd[k]) for k in sd)     # the checkpoint format is untouched
    for bad in ("gpu", "", None, True, 1):
        with pytest.raises(ValueError):
            MultiATGCN(dict(c.config(), hip_dropout=bad), c.data_feature)
    # the offset: a per-model counter, advanced by the number of draws
    assert [m._dropout_offset(1), m._dropout_offset(8), m._dropout_offset(1)] == [0, 1, 9]
    assert callable(m.predict_mc)
