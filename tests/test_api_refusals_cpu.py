"""The refusals of the table, sequence, -dump and path-scoring calls that come before any device is looked at -- what a machine without a GPU
reaches -- as a fixed table of bad calls: the return code and the WHOLE text of mfx_last_error() against tests/golden/api_refusals.json, in the
manner of test_db_refusals_cpu.py.  At least one call of every file that csrc/mfx_api.cpp was split into (mfx_index.cpp, mfx_seq.cpp,
mfx_dump.cpp, mfx_paths.cpp behind the debug entry points) and of what stayed.

Left out, because the device is asked for first (MFX_E_NODEVICE where there is none, and a text that names the number of devices):
mfx_seq_upload and mfx_seq_create with null arguments, mfx_db_stage_begin on an absent path.  The range refusals of mfx_dump_values and the
slot checks of mfx_dump_values_sharded beyond "slot is null" need a sequence object, which needs a device.

The fixture is a recording, not a derivation: `python -m tests.test_api_refusals_cpu` writes it from the library that is built, and it was
written once, from a build of the commit before mfx_api.cpp was split."""
import ctypes as C
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "api_refusals.json")
# what the calls point into
K3, V3, OUT3 = np.array([1, 2, 3], dtype=np.uint64), np.array([1, 2, 3], dtype=np.uint32), np.zeros(3, dtype=np.uint64)
NUL1 = (C.c_void_p * 1)(None)


def _table(m):
    """(name, call): every call is refused; a call that returns a handle returns null"""
    L = m.load_library()
    B = m.binding
    T = []

    def add(name, f, *args):                                     # (an address goes in as the pointer type the binding declared)
        types = f.argtypes or [None] * len(args)
        args = [C.cast(a, t) if isinstance(a, C.c_void_p) and t not in (None, C.c_void_p) else a for a, t in zip(args, types)]
        T.append((name, lambda: f(*args)))

    k3, v3, out3, nul1 = K3, V3, OUT3, NUL1
    p = lambda a: C.c_void_p(a.ctypes.data)
    # ---- mfx_index.cpp
    add("index/create_k0", L.mfx_index_create, 0, 100, 0.0, 0)
    add("index/create_k65", L.mfx_index_create, 65, 100, 0.0, 0)
    add("index/create_lf_k0", L.mfx_index_create_lf, 0, 100, 0.0, 0, 0.5)
    add("index/create_for_seq_k32", L.mfx_index_create_for_seq, 32, 100, 0.0, 0)
    add("index/create_for_seq_lf_k64", L.mfx_index_create_for_seq_lf, 64, 100, 0.0, 0, 0.3)
    add("index/add_read_null", L.mfx_index_add_read, None, p(k3), p(v3), 3, 0, 2**32 - 1, 0)
    add("index/add_asm_null", L.mfx_index_add_asm, None, p(k3), p(v3), 3, 0)
    add("index/count_asm_null", L.mfx_index_count_asm, None, None, None)
    add("index/count_claimed_null", L.mfx_index_count_claimed, None, None, None)
    add("index/claim_seq_null", L.mfx_index_claim_seq, None, None, None)
    add("index/build_for_hist_null", L.mfx_index_build_for_hist, None, None, b"reads.mfxk", 0, 2**32 - 1)
    add("index/build_for_hist_staged_null", L.mfx_index_build_for_hist_staged, None, None, None, 0, 2**32 - 1)
    add("index/load_db_staged_null", L.mfx_index_load_db_staged, None, None, 0, 0, 2**32 - 1)
    add("index/value_null", L.mfx_index_value, None, p(k3), 3, p(v3), p(v3))
    add("index/get_info_null", L.mfx_index_get_info, None, None)
    add("index/export_null", L.mfx_index_export, None, None, None, None, None)
    add("index/place_keys_null", L.mfx_db_place_keys, 21, None, 3, p(out3), 0, 0)
    add("index/place_keys_k31", L.mfx_db_place_keys, 31, p(k3), 3, p(out3), 0, 0)
    add("index/place_keys_k5", L.mfx_db_place_keys, 5, p(k3), 3, p(out3), 0, 0)
    add("index/place_keys_null_before_k", L.mfx_db_place_keys, 31, p(k3), 3, None, 0, 0)
    add("index/stage_begin_null", L.mfx_db_stage_begin, None, 0)
    # ---- mfx_seq.cpp
    add("seq/from_device_null_bases", L.mfx_seq_from_device, 0, None, p(out3), 1, None)
    add("seq/from_device_null_lens", L.mfx_seq_from_device, 0, nul1, None, 1, None)
    add("seq/from_device_negative_device", L.mfx_seq_from_device, -1, None, None, 0, None)
    add("seq/pack_null", L.mfx_seq_pack, None)
    # ---- mfx_dump.cpp
    add("dump/values_null", L.mfx_dump_values, None, None, 0, 0, 10, p(v3), p(v3), None, None)
    add("dump/values_sharded_null", L.mfx_dump_values_sharded, None, None, 1, 0, 0, 10, p(v3), p(v3), None, None)
    add("dump/values_sharded_no_slots", L.mfx_dump_values_sharded, nul1, nul1, 0, 0, 0, 10, p(v3), p(v3), None, None)
    add("dump/values_sharded_null_out", L.mfx_dump_values_sharded, nul1, nul1, 1, 0, 0, 10, None, p(v3), None, None)
    add("dump/values_sharded_slot_null", L.mfx_dump_values_sharded, nul1, nul1, 1, 0, 0, 10, p(v3), p(v3), None, None)
    add("dump/contig_null", L.mfx_dump_contig, None, None, 0, b"chr1", b"out.dump", 0, None, None)
    add("dump/contig_sharded_no_slots", L.mfx_dump_contig_sharded, nul1, nul1, 0, 0, b"chr1", b"out.dump", 0, None, None)
    add("dump/contig_sharded_slot_null", L.mfx_dump_contig_sharded, nul1, nul1, 1, 0, b"chr1", b"out.dump", 0, None, None)
    # ---- the variant modes' device calls, behind the debug entry points (mfx_debug.cpp)
    pt = B.PathTable(b"ACGT\n", [0], [4], [0], [0], [0])
    none = B.TraverseTables(np.zeros(0, dtype=B.TRV_CLUSTER_DTYPE), np.zeros(0, dtype=B.TRV_VARIANT_DTYPE), np.zeros(0, dtype=B.TRV_ALLELE_DTYPE), b"", b"", 5, 0, 0)
    o, ptrs = B._trv_outputs(none)
    T.append(("paths/debug_score_paths_null", lambda: L.mfx_debug_score_paths(None, *(pt.args() + [1, p(v3), p(out3)]))))
    T.append(("paths/debug_score_paths_trv_null", lambda o=o: L.mfx_debug_score_paths_trv(None, *(pt.args() + none.args() + [1, p(v3), p(out3)] + ptrs))))
    # ---- what stayed in mfx_api.cpp
    add("api/eval_create_null", L.mfx_eval_create, None, None, 65536)
    add("api/hist_run_null", L.mfx_hist_run, None, None, None)
    add("api/completeness_null", L.mfx_completeness, None, C.byref(C.c_double(0)), C.byref(C.c_double(0)))
    add("api/gather_rate_small_table", L.mfx_diag_gather_rate, 0, 1024, C.byref(C.c_double(0)))
    return T


def _run(m):
    """name -> [return code, text] of every call of the table"""
    L = m.load_library()
    L.mfx_last_error_code.restype = C.c_int
    out = {}
    for name, call in _table(m):
        assert name not in out, name
        rc = call()
        if not isinstance(rc, int) or rc == 0:                   # a handle: null, and the code is the thread's last
            assert not rc, (name, rc)
            rc = L.mfx_last_error_code()
        assert rc < 0, (name, rc)
        out[name] = [rc, L.mfx_last_error().decode()]
    return out


@pytest.fixture(scope="module")
def got():
    import merfin_amd as m
    return _run(m)


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_is_the_fixtures(got):
    assert sorted(got) == sorted(_golden())


@pytest.mark.parametrize("name", sorted(_golden()) if os.path.exists(GOLDEN) else [])
def test_refusal(got, name):
    rc, text = _golden()[name]
    assert got[name] == [rc, text]
    assert "hip" not in text.lower()


if __name__ == "__main__":                                      # record the fixture from the library that is built
    import sys
    sys.path.insert(0, ROOT)
    import merfin_amd
    rec = _run(merfin_amd)
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d refusals written to %s" % (len(rec), GOLDEN))
