"""Every refusal of the sorted-database calls that comes before a device is looked at -- mfx_db_merge, mfx_db_merge_except, mfx_db_join_completeness,
mfx_db_join_spectrum, mfx_db_diploid, mfx_db_trio, mfx_db_trio_hist, mfx_db_histogram -- as a fixed table of bad calls: the return code and the WHOLE
text of mfx_last_error() against tests/golden/db_refusals.json, the temporary directory in the text replaced by <TMP>.  The tests of the single
calls (test_join_cpu.py, test_trio_cpu.py, test_diploid_cpu.py, test_merge_plan_cpu.py) assert fragments of these texts; this one pins the full
wording and, where two refusals apply to one call, which of them is given.

The fixture is a recording, not a derivation: `python -m tests.test_db_refusals_cpu` writes it from the library that is built, and it was
written once, from a build of the commit before the window drivers left mfx_db.cpp."""
import ctypes as C
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "db_refusals.json")


def _keys(k, n, step):
    return (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(step)) % np.uint64(4 ** min(k, 31))


def _world(m, tmp):
    """the files of the table: a few dozen k-mers each"""
    p = lambda name: os.path.join(tmp, name)
    F = {"tmp": tmp}
    for name, k, n, step in (("a", 21, 40, 7), ("b", 21, 30, 11), ("c", 21, 24, 13), ("k15", 15, 36, 5)):
        keys = np.unique(_keys(k, n, step))
        F[name] = p(name + ".mfxk")
        m.db_write_flat(F[name], k, keys, (np.arange(len(keys), dtype=np.uint32) % 9) + 1)
    F["k32"] = p("k32.mfxk")
    m.db_write_flat(F["k32"], 32, np.array([1, 5, 9], dtype=np.uint64), np.array([1, 2, 3], dtype=np.uint32))
    F["plain"] = p("plain.mfxk")                                  # (not ascending: no sorted form)
    m.db_write_flat(F["plain"], 21, np.array([9, 5, 1], dtype=np.uint64), np.array([1, 2, 3], dtype=np.uint32))
    x = _keys(21, 48, 1234577)                                    # a placed database holds canonical k-mers
    fwd, rc = x.copy(), np.zeros(len(x), dtype=np.uint64)
    for _ in range(21):
        rc = (rc << np.uint64(2)) | ((x & np.uint64(3)) ^ np.uint64(2))
        x = x >> np.uint64(2)
    canon = np.unique(np.minimum(fwd, rc))
    m.db_write_flat(p("canon.mfxk"), 21, canon, np.ones(len(canon), dtype=np.uint32))
    F["placed"] = p("placed.mfxk")
    m.db_convert_placed(p("canon.mfxk"), F["placed"])
    F["text"] = p("print.txt")
    with open(F["text"], "w") as f:
        f.write("ACGTACGTACGTACGTACGTA\t3\n")
    F["meryl"] = p("db.meryl")
    os.mkdir(F["meryl"])
    F["absent"] = p("absent.mfxk")
    F["oa"], F["ob"] = p("A.mfxk"), p("B.mfxk")
    return F


def _table(m, F):
    """(name, call): every call is refused; the names are the fixture's keys"""
    from merfin_amd.binding import DbJoinOpts, DbMergeOpts, DbTrioOpts
    L = m.load_library()
    a, b, c, oa, ob = F["a"], F["b"], F["c"], F["oa"], F["ob"]
    T = []
    add = lambda name, call: T.append((name, call))
    kp = m.KParams(17.3)
    merge = lambda ins, out=oa, **kw: (lambda: m.db_merge(ins, out, **kw))
    exc = lambda ins, nots, out=oa, **kw: (lambda: m.db_merge_except(ins, nots, out, **kw))
    comp = lambda r, s: (lambda: m.db_join_completeness(r, s, kp))
    spec = lambda r, s, **kw: (lambda: m.db_join_spectrum(r, s, **kw))
    dip = lambda r, h1, h2, **kw: (lambda: m.db_diploid(r, h1, h2, **kw))
    trio = lambda mat, pat, child, x=oa, y=ob, **kw: (lambda: m.db_trio(mat, pat, child, x, y, **kw))
    hist = lambda mat, pat, child=None, **kw: (lambda: m.db_trio_hist(mat, pat, child, **kw))
    one = lambda path, **kw: (lambda: m.db_histogram(path, **kw))
    # ---- one bad input, in every call and in more than one place of it
    for kind in ("absent", "meryl", "text", "placed", "plain", "k32"):
        bad = F[kind]
        add("merge/%s" % kind, merge([a, bad]))
        add("merge_except/%s/in" % kind, exc([bad, a], [b]))
        add("merge_except/%s/not" % kind, exc([a], [b, bad]))
        add("completeness/%s/read" % kind, comp(bad, a))
        add("completeness/%s/asm" % kind, comp(a, bad))
        add("spectrum/%s/asm" % kind, spec(a, bad))
        add("diploid/%s/read" % kind, dip(bad, b, c))
        add("diploid/%s/hap2" % kind, dip(a, b, bad))
        add("trio/%s/mat" % kind, trio(bad, b, c, cut_mat=1, cut_pat=1, cut_child=1))
        add("trio/%s/child" % kind, trio(a, b, bad))
        add("trio_hist/%s/pat" % kind, hist(a, bad, c))
        add("histogram/%s" % kind, one(bad))
    # ---- inputs of two k
    add("merge/two_k", merge([a, b, F["k15"]]))
    add("merge_except/two_k/in", exc([F["k15"], a], [b]))
    add("merge_except/two_k/not", exc([a, b], [F["k15"]]))
    add("completeness/two_k", comp(a, F["k15"]))
    add("spectrum/two_k", spec(F["k15"], a))
    add("diploid/two_k/hap1", dip(a, F["k15"], c))
    add("diploid/two_k/hap2", dip(a, b, F["k15"]))
    add("trio/two_k/pat", trio(a, F["k15"], None))
    add("trio/two_k/child", trio(a, b, F["k15"]))
    add("trio_hist/two_k", hist(F["k15"], b))
    # ---- the outputs
    add("merge/out_is_input", merge([a, b], out=b))
    add("merge_except/out_is_input", exc([a, b], [c], out=a))
    add("merge_except/out_is_subtracted", exc([a], [b, c], out=c))
    add("trio/out_a_is_input", trio(a, b, c, x=a, cut_mat=1, cut_pat=1, cut_child=1))
    add("trio/out_b_is_child", trio(a, b, c, y=c, cut_mat=1, cut_pat=1, cut_child=1))
    add("trio/outputs_one_file", trio(a, b, None, x=oa, y=oa, cut_mat=1, cut_pat=1))
    # ---- the options
    add("merge/unknown_op", merge([a, b], op=7))
    add("merge_except/unknown_op", exc([a], [b], op=-1))
    add("merge/min_above_max", merge([a, b], min_count=5, max_count=4))
    add("merge_except/min_above_max", exc([a], [b], min_count=2, max_count=1))
    add("merge/no_inputs", merge([]))
    add("merge_except/too_many", exc([a] * 40, [b] * 40))
    for copies in (0, 65):
        add("spectrum/copies_%d" % copies, spec(a, b, copies=copies))
        add("diploid/copies_%d" % copies, dip(a, b, c, copies=copies))
    for mm in (3, 65537):
        add("spectrum/max_mult_%d" % mm, spec(a, b, max_mult=mm))
        add("diploid/max_mult_%d" % mm, dip(a, b, c, max_mult=mm))
        add("trio/max_mult_%d" % mm, trio(a, b, c, max_mult=mm))
        add("trio_hist/max_mult_%d" % mm, hist(a, b, c, max_mult=mm))
        add("histogram/max_mult_%d" % mm, one(a, max_mult=mm))
    add("trio/cut_child_without_child", trio(a, b, None, cut_mat=1, cut_pat=1, cut_child=2))
    # ---- null arguments (past the Python wrappers)
    enc = lambda s: s.encode()
    arr = lambda *ps: (C.c_char_p * len(ps))(*[None if x is None else enc(x) for x in ps])
    mo, jo, to = DbMergeOpts(0, 0, 2**32 - 1, 0), DbJoinOpts(0, 0, 2**32 - 1, 17.3, 0, None, None, 4, 100), DbTrioOpts(1, 1, 0, 100, 0)
    img, n, t64 = (C.c_uint64 * (6 * 101))(), C.c_uint64(0), (C.c_double * 256)()
    raw = lambda f, *args: (lambda: f(*args))
    add("merge/null_paths", raw(L.mfx_db_merge, None, 2, enc(oa), C.byref(mo), None))
    add("merge/null_path", raw(L.mfx_db_merge, arr(a, None), 2, enc(oa), C.byref(mo), None))
    add("merge/null_out", raw(L.mfx_db_merge, arr(a, b), 2, None, C.byref(mo), None))
    add("merge/null_opts", raw(L.mfx_db_merge, arr(a, b), 2, enc(oa), None, None))
    add("merge_except/null_not_paths", raw(L.mfx_db_merge_except, arr(a), 1, None, 1, enc(oa), C.byref(mo), None, None))
    add("merge_except/null_not_path", raw(L.mfx_db_merge_except, arr(a), 1, arr(b, None), 2, enc(oa), C.byref(mo), None, None))
    add("completeness/null_read", raw(L.mfx_db_join_completeness, None, enc(a), C.byref(jo), t64, t64, None))
    add("completeness/null_opts", raw(L.mfx_db_join_completeness, enc(a), enc(b), None, t64, t64, None))
    add("completeness/null_result", raw(L.mfx_db_join_completeness, enc(a), enc(b), C.byref(jo), t64, None, None))
    add("spectrum/null_asm", raw(L.mfx_db_join_spectrum, enc(a), None, C.byref(jo), img, C.byref(n), None))
    add("spectrum/null_image", raw(L.mfx_db_join_spectrum, enc(a), enc(b), C.byref(jo), None, C.byref(n), None))
    add("diploid/null_hap2", raw(L.mfx_db_diploid, enc(a), enc(b), None, C.byref(jo), img, img, C.byref(n), C.byref(m.binding.DbDiploidStats()), None, None))
    add("diploid/null_stats", raw(L.mfx_db_diploid, enc(a), enc(b), enc(c), C.byref(jo), img, img, C.byref(n), None, None, None))
    add("diploid/total_without_undrcpy", raw(L.mfx_db_diploid, enc(a), enc(b), enc(c), C.byref(jo), img, img, C.byref(n), C.byref(m.binding.DbDiploidStats()), t64, None))
    add("trio/null_mat", raw(L.mfx_db_trio, None, enc(b), None, enc(oa), enc(ob), C.byref(to), None, None))
    add("trio/null_out_b", raw(L.mfx_db_trio, enc(a), enc(b), None, enc(oa), None, C.byref(to), None, None))
    add("trio/null_opts", raw(L.mfx_db_trio, enc(a), enc(b), None, enc(oa), enc(ob), None, None, None))
    add("trio_hist/null_image", raw(L.mfx_db_trio_hist, enc(a), enc(b), None, 100, None, None, 0))
    add("trio_hist/null_pat", raw(L.mfx_db_trio_hist, enc(a), None, None, 100, img, None, 0))
    add("histogram/null_path", raw(L.mfx_db_histogram, None, 100, img, None, 0))
    add("histogram/null_row", raw(L.mfx_db_histogram, enc(a), 100, None, None, 0))
    # ---- two refusals at once: which one is given
    add("first/merge/unknown_op_before_absent", merge([a, F["absent"]], op=9))
    add("first/merge/min_above_max_before_out_is_input", merge([a, b], out=a, min_count=9, max_count=1))
    add("first/merge/two_k_before_out_is_input", merge([a, F["k15"]], out=F["k15"]))
    add("first/merge/two_k_before_absent", merge([a, F["k15"], F["absent"]]))
    add("first/merge_except/out_is_input_before_absent_subtracted", exc([a, b], [F["absent"]], out=b))
    add("first/merge_except/out_is_subtracted_before_absent", exc([a], [b, F["absent"]], out=b))
    add("first/merge_except/too_many_before_unknown_op", exc([a] * 40, [b] * 40, op=9))
    add("first/completeness/absent_before_two_k", comp(F["k15"], F["absent"]))
    add("first/completeness/plain_before_two_k", comp(F["k15"], F["plain"]))
    add("first/spectrum/copies_before_absent", spec(F["absent"], b, copies=0))
    add("first/spectrum/copies_before_max_mult", spec(a, b, copies=0, max_mult=3))
    add("first/diploid/two_k_before_absent", dip(a, F["k15"], F["absent"]))
    add("first/diploid/max_mult_before_meryl", dip(F["meryl"], b, c, max_mult=3))
    add("first/trio/k32_before_absent", trio(F["k32"], F["absent"], None))
    add("first/trio/max_mult_before_cut_child", trio(a, b, None, cut_mat=1, cut_pat=1, cut_child=2, max_mult=3))
    add("first/trio/cut_child_before_absent", trio(F["absent"], b, None, cut_mat=1, cut_pat=1, cut_child=2))
    add("first/trio/out_is_input_before_outputs_one_file", trio(a, b, None, x=a, y=a, cut_mat=1, cut_pat=1))
    add("first/trio/two_k_before_out_is_input", trio(a, F["k15"], None, x=a, cut_mat=1, cut_pat=1))
    add("first/trio_hist/placed_before_two_k", hist(F["k15"], F["placed"]))
    return T


def _run(m, tmp):
    """name -> [return code, text] of every call of the table"""
    L = m.load_library()
    F = _world(m, tmp)
    kept = {p: open(F[p], "rb").read() for p in ("a", "b", "c", "k15")}
    out = {}
    for name, call in _table(m, F):
        assert name not in out, name
        try:
            rc = call()
        except m.MfxError as e:
            rc = e.code
        assert isinstance(rc, int) and rc < 0, (name, rc)         # (a call that went on would end in a HIP error: this machine may have no device)
        out[name] = [rc, L.mfx_last_error().decode().replace(tmp, "<TMP>")]
    assert {p: open(F[p], "rb").read() for p in kept} == kept      # no refused call has touched an input that was named as an output
    assert not any(os.path.exists(F[o] + s) for o in ("oa", "ob") for s in ("", ".blocks"))
    return out


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    import merfin_amd as m
    return _run(m, str(tmp_path_factory.mktemp("refusals")))


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
    import tempfile
    sys.path.insert(0, ROOT)
    import merfin_amd
    with tempfile.TemporaryDirectory() as d:
        rec = _run(merfin_amd, d)
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d refusals written to %s" % (len(rec), GOLDEN))
