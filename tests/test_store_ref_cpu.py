"""CPU: the store pass of the row-block SDDMM, without a device.

* the host-only run cutting (csrc/rb_schedule.cpp rb_cut_runs, through the debug export
  bsmr_debug_rb_runs) against its numpy restatement (store_cases.cut_runs_ref) on every edge of
  the cut: sequences of 1, 63, 64, 65, 128 and 129 consecutive positions, alternating positions,
  an empty item, exactly NT and NT + 1 runs for both workgroup sizes, the packing of a run that
  reaches slot 65534; the same edges through a stand-alone build of the function under ASan and
  UBSan (tests/rb_runs_main.cpp);
* identity data (sddmm_cases.identity_data): every stored entry is 4096 row + column, exactly, in
  fp32, fp16 and bf16 and under random summation orders;
* a numpy emulation of the two store forms (store_cases.store_by_runs / store_by_positions, written
  from the kernel's comments: runs dealt w + NW lane in steps of four; trips of 8 NT) over
  host-built layouts: unmutated it reproduces identity data exactly, and each of six mutations of
  the kind a subtly wrong kernel or table would show fails assert_exact on identity data;
* the classifier of test_gpu_sddmm_store_float64.py (store_cases.classify) on host-built layouts
  of every STORE_CASES row with original-order row blocks (their layout follows from the CSR
  alone: test_rb_schedule_cpu.py), and one case with a knob changed, whose evidence assertion then
  fails while its numerics would not.

The host-built layout (model_dump): the geometry and the scheduler through their device-free
exports (as test_rb_schedule_cpu.csr_layout), the item's slots sorted by CSR position, the run
cutting through bsmr_debug_rb_runs and the pair decision through bsmr_debug_rb_form: the same
functions build_rowblock_layout calls, in its order.

Which mutations grid data alone misses (test_what_grid_data_misses): four of the six leave
entries unwritten, which any data catches through the NaN that P starts as. The two that put a
wrong slot's value into a written entry (a lane equal to len stores; the slot base of the
neighbouring run) are caught by grid data only where the two entries' values differ. On the
suite's grid data at K = 128 about one pair of entries in 14,000 has equal values (7,841
distinct values among 11,328 entries); the six bulk mutations move hundreds of entries and so
none of them passes on grid data here, but a single misplaced store, the off-by-one kind, passes
on grid data once in about 14,000 times and a swap of two equal-valued entries (the test builds
one) passes always. On identity data every entry has its
own value: no misplaced store passes.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sddmm_cases as S
import store_cases as SC
from bsmr import BF16, F16, F32
from gpu_util import store_constants
from test_launch_select_cpu import rb_form
from test_rb_schedule_cpu import GEOM, geometry, schedule

CUS = 256  # the MI355X's compute units
CONST = store_constants()  # PAIR_RUNS_PER_WAVE, XCD_BUCKETS, RB_RUN_MAX as the library has them


def test_constants_come_from_the_library():
    """The numpy store passes are written for waves of 64 lanes and runs of at most 64; the pair
    classes come from the library's own PAIR_RUNS_PER_WAVE and XCD_BUCKETS (model_dump)."""
    assert CONST["run_max"] == SC.RUN_MAX == 64
    assert CONST["prpw"] >= 1 and CONST["xcds"] >= 1


# ---- the run cutting ------------------------------------------------------------------------------

def _seq(start, n):
    return np.arange(start, start + n)


def _edge_items():
    """name: (sorted positions, ient (n x 2), NT)."""
    out = {}
    for n in (1, 63, 64, 65, 128, 129):
        out[f"consecutive_{n}"] = (_seq(7, n), [(0, n)], 512)
    out["alternating"] = (np.arange(0, 400, 2), [(0, 200)], 512)
    out["empty_item_between"] = (np.concatenate([_seq(0, 70), _seq(100, 3)]), [(0, 70), (70, 0), (70, 3)], 512)
    out["no_items"] = (np.zeros(0), np.zeros((0, 2)), 512)
    for NT in (512, 1024):
        out[f"exactly_nt_runs_{NT}"] = (np.arange(0, 2 * NT, 2), [(0, NT)], NT)
        out[f"nt_plus_one_runs_{NT}"] = (np.arange(0, 2 * NT + 2, 2), [(0, NT + 1)], NT)
        # a second item that fits does not rescue the table
        out[f"one_item_over_{NT}"] = (np.arange(0, 2 * NT + 12, 2), [(0, 5), (5, NT + 1)], NT)
    # 65535 entries (outCap < 65536), slots 0 .. 65534, in the fewest runs there can be: 1024, the
    # last one {slot 65472, length 63} reaching slot 65534, the highest a run word's 16 bits address
    out["slot_65534"] = (_seq(9, 65535), [(0, 65535)], 1024)
    # runs of mixed lengths over several items, in an order that is not the slot order of the table
    rng = np.random.default_rng(3)
    pos = np.sort(rng.choice(3600, 3000, replace=False))  # ~500 runs
    out["random_mixed"] = (pos, [(0, 900), (900, 0), (900, 1500), (2400, 600)], 512)
    return out


EDGES = _edge_items()


@pytest.mark.parametrize("name", sorted(EDGES))
def test_run_cutting_matches_the_restatement(name):
    pos, ient, NT = EDGES[name]
    ient = np.asarray(ient, np.uint32).reshape(-1, 2)
    lib, ref = SC.cut_runs(pos, ient, NT), SC.cut_runs_ref(pos, ient, NT)
    assert lib["fits"] == ref["fits"]
    assert np.array_equal(lib["itemRuns"], ref["itemRuns"])
    assert np.array_equal(lib["runs"], ref["runs"])
    if lib["fits"]:  # the runs tile every item's slots in order, and name its positions
        for (e0, n), (r0, nr) in zip(ient.astype(np.int64), lib["itemRuns"].astype(np.int64)):
            r = lib["runs"][r0:r0 + nr].astype(np.int64)
            ln = r[:, 1] >> 16
            assert (ln >= 1).all() and (ln <= 64).all() and ln.sum() == n
            assert np.array_equal(r[:, 1] & 0xFFFF, np.cumsum(ln) - ln)
            assert np.array_equal(np.concatenate([p + np.arange(k) for p, k in zip(r[:, 0], ln)] or
                                                 [np.zeros(0, np.int64)]), np.asarray(pos, np.int64)[e0:e0 + n])


def test_run_cutting_named_edges():
    cut = lambda name: SC.cut_runs(*EDGES[name][:2], EDGES[name][2])  # noqa: E731
    lens = lambda t: [int(w) >> 16 for w in t["runs"][:, 1]]  # noqa: E731
    assert lens(cut("consecutive_63")) == [63] and lens(cut("consecutive_64")) == [64]
    assert lens(cut("consecutive_65")) == [64, 1] and lens(cut("consecutive_128")) == [64, 64]
    assert lens(cut("consecutive_129")) == [64, 64, 1]
    assert set(lens(cut("alternating"))) == {1} and len(cut("alternating")["runs"]) == 200
    t = cut("empty_item_between")
    assert [tuple(x) for x in t["itemRuns"]] == [(0, 2), (2, 0), (2, 1)]
    for NT in (512, 1024):
        assert cut(f"exactly_nt_runs_{NT}")["fits"] and len(cut(f"exactly_nt_runs_{NT}")["runs"]) == NT
        for name in (f"nt_plus_one_runs_{NT}", f"one_item_over_{NT}"):
            t = cut(name)
            assert not t["fits"] and len(t["runs"]) == 0 and int(t["itemRuns"][-1, 1]) == NT + 1
    # (512 threads take NT + 1 = 513 runs no more than 1024 threads take 1025, but 1024 take 513)
    assert SC.cut_runs(*EDGES["nt_plus_one_runs_512"][:2], 1024)["fits"]
    t = cut("slot_65534")
    assert t["fits"] and len(t["runs"]) == 1024
    assert tuple(int(x) for x in t["runs"][-1]) == (9 + 65472, 65472 | (63 << 16))
    assert (int(t["runs"][-1, 1]) & 0xFFFF) + (int(t["runs"][-1, 1]) >> 16) - 1 == 65534


def test_run_cutting_does_not_depend_on_the_host_threads():
    pos, ient, NT = EDGES["random_mixed"]
    many = (np.concatenate([pos + 6000 * k for k in range(1200)]),
            np.concatenate([np.asarray(ient) + [3000 * k, 0] for k in range(1200)]))  # 4800 items: threaded
    a, b = SC.cut_runs(*many, NT, threads=1), SC.cut_runs(*many, NT, threads=7)
    assert a["fits"] and np.array_equal(a["runs"], b["runs"]) and np.array_equal(a["itemRuns"], b["itemRuns"])
    assert np.array_equal(a["runs"], SC.cut_runs_ref(*many, NT)["runs"])


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sddmm-gpu_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/rb_runs_main.cpp with rb_schedule.cpp and knobs.cpp under ASan and UBSan (a program of
    its own, as the softmax item list has: tests/test_softmax_items_cpu.py)."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("rb_runs_asan")
    exe = str(d / "rb_runs_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-pthread", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "rb_runs_main.cpp"), os.path.join(CSRC, "rb_schedule.cpp"),
           os.path.join(CSRC, "knobs.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr:
            pytest.skip("sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
        raise AssertionError(r.stderr)
    return exe, d


def _fnv(words):
    h = 0xcbf29ce484222325
    for b in np.ascontiguousarray(words, "<u4").tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("name", sorted(EDGES))
def test_sanitized_standalone_build_agrees(driver, name):
    exe, d = driver
    pos, ient, NT = EDGES[name]
    ient = np.asarray(ient, np.uint32).reshape(-1, 2)
    threads = 3
    path = str(d / f"{name}.txt")
    with open(path, "w") as f:
        f.write(f"{NT} {threads} {len(ient)}\n" + " ".join(map(str, ient.reshape(-1).tolist())) + "\n" +
                " ".join(str(int(p)) for p in pos) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    t = SC.cut_runs(pos, ient, NT, threads=threads)
    words = np.concatenate([t["itemRuns"].reshape(-1), t["runs"].reshape(-1)])
    assert r.stdout.split() == [str(int(t["fits"])), str(len(t["runs"])), f"{_fnv(words):016x}"]


# ---- identity data --------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, F16, BF16])
@pytest.mark.parametrize("K", [16, 32, 128, 200, 1024])
def test_identity_data_is_exact(K, dtype):
    pat = S.pattern("zipf")  # 517 x 4000
    M, N, rp, ci = pat
    A, B = S.identity_data(M, N, K)
    assert np.array_equal(S.as_seen(A, dtype), A) and np.array_equal(S.as_seen(B, dtype), B)
    want = S.identity_values(pat)
    ref, _ = S.sddmm_ref(pat, A, B, dtype)
    assert np.array_equal(ref, want) and len(np.unique(want)) == len(want)
    # fp32 accumulation in three random k orders and one pairwise order: still exact
    rows, cols = S.entry_rows(M, rp)[::7], np.asarray(ci, np.int64)[::7]
    prod = A[rows] * B[cols]
    rng = np.random.default_rng(K)
    for _ in range(3):
        acc = np.zeros(len(rows), np.float32)
        for k in rng.permutation(K):
            acc += prod[:, k]
        assert np.array_equal(acc.astype(np.float64), want[::7])
    assert np.array_equal(prod.sum(axis=1, dtype=np.float32).astype(np.float64), want[::7])


def test_identity_data_at_the_largest_pattern():
    A, B = S.identity_data(4096, 4096, 16)
    assert float(A[4095] @ B[4095]) == 4096.0 * 4095 + 4095 < 2 ** 24
    assert np.abs(A).max() <= 4096 and np.abs(B).max() <= 4096


# ---- host-built layouts ---------------------------------------------------------------------------

def model_dump(pat, K, dtype, tuning, cus=CUS):
    """(dump, sortedPos) of the whole-plan original-order row-block layout of `pat`, built on the
    host from the same exports in build_rowblock_layout's order (module docstring). dump: the
    dict of gpu_util.rb_store plus "pairs" (the launch's form)."""
    assert tuning.get("orig_rows") == 1
    M, N, rp, ci = pat
    nnz = len(ci)
    row_bytes = K * (4 if dtype == F32 else 2)
    g = geometry(row_bytes, M, nnz, N, nnz, cus, orig=True, tuning=tuning)
    G = dict(zip(GEOM, (int(v) for v in g)))
    block = S.entry_rows(M, rp) // G["RB"]
    order = np.lexsort((np.asarray(ci, np.int64), block))  # stable, like the device sort
    rb_end = np.cumsum(np.bincount(block, minlength=G["nRB"]))[:G["nRB"]]
    s = schedule(np.asarray(ci)[order], rb_end, g, N, tuning=tuning)
    items, ends, pieces = s["items"], s["ends"], s["pieces"]
    n = len(items)
    real = ~((items[:, 1] == items[:, 2]) & (items[:, 3] == ends))
    ient = np.zeros((n, 2), np.uint32)
    for i in np.nonzero(real)[0]:  # an item's entries are contiguous: from its first piece's on
        ient[i] = (pieces[items[i, 3]:ends[i], 0].min(), s["stat"][i, 2])
    spos = np.zeros(nnz, np.uint32)
    for e0, ln in ient.astype(np.int64):
        spos[e0:e0 + ln] = np.sort(order[e0:e0 + ln])
    staged = bool(G["staged"])
    d = dict(outLds=G["lds"] if staged else 0, outCap=G["outCap"] if staged else 0, outRuns=False,
             outPacked=False, NT=G["NT"], nItems=n, prpw=CONST["prpw"], xcds=CONST["xcds"], ent=ient[:, 1].copy(),
             nruns=np.zeros(n, np.uint32), longest=None, shortest=None, itemEnt=ient, itemRuns=None, runs=None,
             sortedPos=spos, rb=items[:, 0].copy(), real=real)
    if staged and not tuning.get("diag", 0) & 8192 and G["outCap"] < 65536:
        t = SC.cut_runs(spos, ient, G["NT"])
        if t["fits"]:
            d.update(outRuns=True, itemRuns=t["itemRuns"], runs=t["runs"], nruns=t["itemRuns"][:, 1].copy())
    form = rb_form(dict(rowBytes=row_bytes, NT=G["NT"], nItems=n, nTilesKept=0, outLds=d["outLds"],
                        outRuns=int(d["outRuns"]), dynBatches=s["dyn"]), tuning)
    d["pairs"] = bool(form["pairs"])
    return d, spos


# a pattern small enough to emulate store by store, on a model device of 8 compute units (16
# workgroup slots, so its items are as large as the MI355X's are on `band`)
MINI = {"R": S.band_scatter(272, 1024, 16, 420, 18, seed=5),
        "S": S.shuffled(S.band_scatter(528, 1024, 16, 700, 20, seed=5))}
MINI_TUNING = dict(SC.BAND, rb_rows=16)


@pytest.fixture(scope="module")
def mini():
    """{form: (dump, sortedPos)} of MINI: a sorted pattern (run table) and a shuffled one (sortedPos)."""
    out = {f: model_dump(MINI[f], 128, F32, MINI_TUNING, cus=8) for f in MINI}
    assert out["R"][0]["outRuns"] and out["S"][0]["outLds"] and not out["S"][0]["outRuns"]
    return out


def test_mini_layouts_have_what_the_mutations_need(mini):
    ev, _ = SC.classify(mini["R"][0], False)
    assert {"R", "R-steps", "R-64", "R-idle"} <= ev, ev
    ev, facts = SC.classify(mini["S"][0], False)
    assert {"S", "S-trips", "S-small"} <= ev, (ev, facts)
    rule, most = SC.host_rule(mini["S"][0])
    assert not rule and most > mini["S"][0]["NT"]


@pytest.mark.parametrize("form", ["R", "S"])
@pytest.mark.parametrize("reverse", [False, True])
def test_emulation_reproduces_identity_data(mini, form, reverse):
    dump, spos = mini[form]
    want = S.identity_values(MINI[form])
    P = SC.emulate(dump, spos, want, reverse=reverse)
    assert np.isnan(P[-1]), "a store past P[nnz)"
    S.assert_exact(P[:-1].astype(np.float32), want, f"emulated form {form}")


def _fails(P, want, what):
    try:
        S.assert_exact(P[:len(want)].astype(np.float32), want, what)
    except AssertionError as e:
        return str(e)
    return None


def _rejected(dump, spos, values, mutation):
    """The assert_exact message of the first item order (forwards, backwards: workgroups are not
    ordered, so a result that is wrong in either order is wrong) in which the mutated emulation
    fails, or None."""
    for reverse in (False, True):
        msg = _fails(SC.emulate(dump, spos, values, mutation=mutation, reverse=reverse), values, mutation)
        if msg:
            return msg
    return None


def _form_of(mutation):
    return "S" if mutation == "second_trip_dropped" else "R"


@pytest.mark.parametrize("mutation", SC.MUTATIONS)
def test_mutation_fails_on_identity_data(mini, mutation):
    form = _form_of(mutation)
    dump, spos = mini[form]
    want = S.identity_values(MINI[form])
    msg = _rejected(dump, spos, want, mutation)
    assert msg is not None and ("differ from the exact result" in msg or "never written" in msg), msg


def _grid_values(pat, K=128):
    M, N, _, _ = pat
    A = S.grid_data(M * K, 101).reshape(M, K)
    B = S.grid_data(N * K, 202).reshape(N, K)
    return S.sddmm_ref(pat, A, B)[0]


def test_what_grid_data_misses(mini):
    """Module docstring: the bulk mutations all fail on grid data too (four of them through
    unwritten entries alone), but grid values repeat, so one misplaced store can pass: a swap of
    two equal-valued entries of one item passes on grid data and fails on identity data."""
    missed = []
    for mutation in SC.MUTATIONS:
        form = _form_of(mutation)
        dump, spos = mini[form]
        grid = _grid_values(MINI[form])
        msg = _rejected(dump, spos, grid, mutation)
        if msg is None:
            missed.append(mutation)
        elif mutation not in ("lane_equal_to_len_stores", "slot_of_neighbouring_run"):
            assert "never written" in msg
    print("mutations that pass on grid data:", missed)
    assert missed == []
    dump, spos = mini["R"]
    grid, ident = _grid_values(MINI["R"]), S.identity_values(MINI["R"])
    _, inv, cnt = np.unique(grid, return_inverse=True, return_counts=True)
    pairs_equal = float((cnt * (cnt - 1)).sum()) / (len(grid) * (len(grid) - 1))
    print(f"grid data: {len(cnt)} distinct values among {len(grid)} entries, "
          f"a pair is equal with probability {pairs_equal:.2e}")
    assert pairs_equal > 0  # (about 1 in 14,000 at K = 128: grid values repeat)
    # two slots of one item whose grid values are equal, swapped: the kind of error one misplaced
    # store makes
    for e0, n in np.asarray(dump["itemEnt"], np.int64):
        v = grid[spos[e0:e0 + n]]
        _, first, c = np.unique(v, return_index=True, return_counts=True)
        if (c > 1).any():
            a = int(first[np.argmax(c > 1)])
            b = int(np.nonzero(v == v[a])[0][1])
            break
    else:
        raise AssertionError("no item with two equal grid values")
    swapped = spos.copy()
    swapped[e0 + a], swapped[e0 + b] = spos[e0 + b], spos[e0 + a]
    # (the slots' values are taken from the swapped order, the stores go to the true positions)
    for values, passes in ((grid, True), (ident, False)):
        P = np.full(len(values), np.nan)
        P[spos] = values[swapped]
        assert (_fails(P, values, "swap") is None) == passes


# ---- the classifier -------------------------------------------------------------------------------

MODEL_CASES = [c.name for c in SC.STORE_CASES if c.model]


@pytest.fixture(scope="module")
def model_of():
    cache = {}

    def get(case, **changed):
        key = (case.name, tuple(sorted(changed.items())))
        if key not in cache:
            cache[key] = model_dump(S.pattern(case.pattern), case.K, case.dtype, dict(case.tuning, **changed))
        return cache[key]
    return get


@pytest.mark.parametrize("name", MODEL_CASES)
def test_case_shows_its_evidence_on_the_host_model(name, model_of):
    case = SC.STORE_BY_NAME[name]
    dump, _ = model_of(case)
    assert dump["pairs"] == case.pairs
    ev, facts = SC.classify(dump, dump["pairs"])
    print(f"STORE {name}: {sorted(ev)} {facts}")
    assert case.evidence <= ev, (sorted(case.evidence - ev), facts)
    if "S" in case.evidence:
        rule, most = SC.host_rule(dump)
        assert not rule and most > dump["NT"]


@pytest.mark.parametrize("name,changed,lost", [
    # items capped at a fifth of a slot's share: no item has more runs than threads, the run table
    # comes back (and with it the pairs that pair_min_items = 0 allows)
    ("pos_band_rb64", {"piece_weight": 4.0, "item_cap": 0.2}, {"S", "S-trips", "S-small"}),
    # the default piece weight: form S still, but no item of a second trip
    ("pos_band_rb64", {"piece_weight": 4.0}, {"S-trips"}),
    # the same pairs without the large items (default piece weight): no slot tail under the partner
    ("pair_band_rb144", {"piece_weight": 4.0}, {"P-reg-stage-tail"}),
    # pairs refused (the default threshold): the same layout runs as single items
    ("pair_band_rb288", {"pair_min_items": 4096}, {"P", "P-reg-stage", "P-plain-stage"}),
    ("runs_band_rb144", {"rb_rows": 16}, {"R-tail"}),
])
def test_changed_knobs_fail_the_evidence_not_the_numerics(name, changed, lost, model_of):
    """The evidence assertion is what notices a layout that fell back to another form: the emulated
    result of the changed layout is still exact."""
    case = SC.STORE_BY_NAME[name]
    dump, spos = model_of(case, **changed)
    ev, facts = SC.classify(dump, dump["pairs"])
    assert lost <= case.evidence - ev, (sorted(ev), facts)
    assert not case.evidence <= ev  # (what test_store_case asserts, failing)
    want = S.identity_values(S.pattern(case.pattern))
    if not dump["outRuns"]:  # (form S emulates in bulk; the run form store by store, too slow here)
        S.assert_exact(SC.emulate(dump, spos, want)[:-1].astype(np.float32), want, name)


def test_classifier_on_hand_made_pairs():
    """Two XCD lists worth of hand-made items: every pair class from the table alone."""
    X, NT = CONST["xcds"], 512
    n = 4 * X  # list positions 0 .. 3: workgroups (0, 1) and (2, 3) of every XCD
    real = np.ones(n, bool)
    rb = np.zeros(n, np.uint32)
    nruns = np.full(n, 5, np.uint32)
    ent = np.full(n, 40, np.uint32)
    rb[1 * X + 0] = 1           # XCD 0, first pair: another row block -> P-reg-stage
    ent[0 * X + 0] = 1500       # ... by a first item past half of outCap -> P-reg-stage-tail
    lim = NT // 64 * CONST["prpw"]  # the register path's limit: NW x PAIR_RUNS_PER_WAVE runs
    nruns[0 * X + 1] = lim + 1  # XCD 1, first pair: over the limit -> P-plain-same
    nruns[2 * X + 1] = lim + 1
    rb[3 * X + 1] = 2           # XCD 1, second pair: P-plain-stage
    real[3 * X + 2] = False     # XCD 2, second pair: the partner is padding -> P-last
    real[2 * X + 3] = real[3 * X + 3] = False  # XCD 3: an idle workgroup
    dump = dict(outLds=4096, outCap=2044, outRuns=True, NT=NT, prpw=CONST["prpw"], xcds=X, real=real, rb=rb, nruns=nruns,
                ent=ent, itemRuns=None, runs=None)
    ev, _ = SC.classify(dump, True)
    assert ev == {"NT512", "P", "P-reg-same", "P-reg-stage", "P-reg-stage-tail", "P-plain-same",
                  "P-plain-stage", "P-last"}
    nruns[0 * X + 1] = lim      # exactly NW x PAIR_RUNS_PER_WAVE: still the register path
    ev, _ = SC.classify(dump, True)
    assert "P-plain-same" not in ev


def test_wave_run_counts():
    assert list(SC.wave_run_counts(0, 8)) == [0] * 8
    assert list(SC.wave_run_counts(5, 8)) == [1] * 5 + [0] * 3
    assert list(SC.wave_run_counts(35, 8)) == [5, 5, 5, 4, 4, 4, 4, 4]
    assert SC.wave_run_counts(512, 8).tolist() == [64] * 8
