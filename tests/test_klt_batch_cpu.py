"""hip_klt's batch form (include/ofps_hip.h N3b): what tests/klt_batch_cases.py promises, asserted of the NumPy restatement alone -- the GPU
test must not pass on inputs that separate nothing -- and the statements of the new entry points and options.  No GPU."""
import os
import re

import numpy as np

import ffi_parse
import indep_klt as ik
import klt_batch_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["ofps_hip_klt_flow_batch", "ofps_hip_klt_flow_batch_dev", "ofps_hip_set_batch_decoder", "ofps_hip_get_batch_decoder"]
NEW_OPTIONS = ["OFPS_HIP_KLT_CELL", "OFPS_HIP_KLT_SCORE_RADIUS", "OFPS_HIP_KLT_MIN_SCORE", "OFPS_HIP_KLT_MIN_EIG", "OFPS_HIP_KLT_MAX_RESIDUAL",
               "OFPS_HIP_BATCH_DECODER", "OFPS_HIP_KLT_LEVELS", "OFPS_HIP_KLT_RADIUS", "OFPS_HIP_KLT_ITERS"]


def _statuses(items):
    return [set(np.unique(e["slots"][:, 5]).tolist()) for e in items]


def test_small_sequence_keeps_what_the_cases_say():
    fr = bc.sequence(bc.SMALL)
    assert fr.shape == (6, 96, 128)
    assert ik.slot_grid(128, 96, 16) == (8, 6) and ik.slot_grid(128, 96, 8) == (16, 12)
    for params in bc.SMALL_SETS:
        items = bc.expect(bc.SMALL, params)
        counts = tuple(int(e["count"]) for e in items)
        print(params, counts, _statuses(items))
        assert counts == bc.SMALL_KEPT[params], params
        for e in items:
            assert len(e["records"]) == e["count"] == int((e["slots"][:, 5] == ik.ST_KEPT).sum())


def test_small_sequence_reaches_the_statuses_the_cases_name():
    st = _statuses(bc.expect(bc.SMALL, bc.SMALL_SETS[0]))
    assert ik.ST_LEFT in st[1] and ik.ST_LEFT in st[4]
    every = set().union(*_statuses(bc.expect(bc.SMALL, bc.SMALL_SETS[1])))
    assert ik.ST_FLAT in every and ik.ST_RESIDUAL in every
    flat = bc.expect(bc.SMALL, bc.ALL_FLAT)
    assert all(set(np.unique(e["slots"][:, 5]).tolist()) <= {ik.ST_NONE, ik.ST_FLAT} and e["count"] == 0 for e in flat)
    few = set().union(*_statuses(bc.expect(bc.SMALL, bc.FEW)))
    assert {ik.ST_NONE, ik.ST_LEFT, ik.ST_RESIDUAL} <= few
    assert all(e["count"] < 4 for e in bc.expect(bc.SMALL, bc.FEW))


def test_items_are_pairwise_distinct():
    """an implementation that mixes up items, pitches or counts cannot pass: no two items of a set answer alike (the all-flat set apart)"""
    for params in bc.SMALL_SETS:
        if params == bc.ALL_FLAT:
            continue
        for ref_mode in (0, 1) if params in bc.KEY_SETS else (0,):
            items = bc.expect(bc.SMALL, params, ref_mode)
            keys = [e["slots"].tobytes() for e in items]
            assert len(set(keys)) == len(keys), (params, ref_mode)
            recs = [e["records"].tobytes() for e in items]
            assert len(set(recs)) == len(recs), (params, ref_mode)
    # key mode differs from the chain in every item but the first
    for params in bc.KEY_SETS:
        chain, key = bc.expect(bc.SMALL, params, 0), bc.expect(bc.SMALL, params, 1)
        assert chain[0]["slots"].tobytes() == key[0]["slots"].tobytes()
        assert all(chain[k]["slots"].tobytes() != key[k]["slots"].tobytes() for k in range(1, 5))


def test_big_sequence_needs_a_second_compaction_round():
    assert ik.slot_grid(384, 224, 8) == (48, 28) and 48 * 28 == 1344 > 1024
    items = bc.expect(bc.BIG, bc.BIG_SETS[0])
    assert tuple(int(e["count"]) for e in items) == bc.BIG_KEPT[bc.BIG_SETS[0]]
    assert items[0]["slots"].tobytes() != items[1]["slots"].tobytes()
    # kept slots on both sides of slot 1,024: the second round has records to move and a base to carry over
    for e in items:
        kept = np.flatnonzero(e["slots"][:, 5] == ik.ST_KEPT)
        assert (kept < 1024).any() and (kept >= 1024).any()


def test_header_ctypes_table_rust_block_and_options_declare_the_batch_form():
    hdr = ffi_parse.header_signatures()
    rs = ffi_parse.rust_signatures()
    from ofps_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in hdr, name + " is not in include/ofps_hip.h"
        assert name in _lib.PROTOTYPES, name + " is not in ofps_amd/_lib.py"
        assert name in rs, name + " is not in INTEGRATION.md's Rust block"
        ret, args = hdr[name]
        res, cargs = _lib.PROTOTYPES[name]
        assert len(args) == len(cargs) == len(rs[name][1]), name
        for a, c, r in zip(args, cargs, rs[name][1]):
            assert ffi_parse.same_class(a, ffi_parse.ctypes_class(c), lp64=True), (name, a, c)
            assert ffi_parse.same_class(a, r), (name, a, r)
    assert len(hdr["ofps_hip_klt_flow_batch_dev"][1]) == 14 and hdr["ofps_hip_klt_flow_batch_dev"][1][6] == "usize"
    text = open(os.path.join(ROOT, "include", "ofps_hip.h")).read()
    assert re.search(r"OFPS_HIP_BATCH_DECODER_SAD\s*=\s*0\s*,\s*OFPS_HIP_BATCH_DECODER_KLT\s*=\s*1", text)
    assert "N3b" in text
    # the additions are additive: the version the header, the Rust block and the library state stays the one every binding was written against
    version = int(re.search(r"#define\s+OFPS_HIP_API_VERSION\s+(\d+)", text).group(1))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"pub const OFPS_HIP_API_VERSION: c_int = (\d+);", integration).group(1)) == version
    ctx_src = open(os.path.join(ROOT, "ofps_amd", "csrc", "ctx.hip")).read()
    names = re.search(r"kOptionNames\[\]\s*=\s*\{(.*?)\};", ctx_src, re.S).group(1)
    for opt in NEW_OPTIONS:
        assert '"' + opt + '"' in names, opt + " is not in the option list"
        assert ctx_src.count('"' + opt + '"') >= 2, opt + " is not handled by apply_option"
        assert opt in integration, opt + " is not in INTEGRATION.md"
    from ofps_amd.runtime import HipContext, MultiDevice
    assert (HipContext.BATCH_DECODER_SAD, HipContext.BATCH_DECODER_KLT) == (0, 1)
    for fn in ("klt_flow_batch", "klt_flow_batch_dev", "set_batch_decoder", "get_batch_decoder", "batch_record_capacity"):
        assert callable(getattr(HipContext, fn))
    assert callable(MultiDevice.batch_record_capacity)
