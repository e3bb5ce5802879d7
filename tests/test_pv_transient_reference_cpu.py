"""CPU-side checks of the transient-preserving stretch's definition (tests/pv_transient_reference.py) and of the library's host half
against it: the two statements of the stage agree within the lock family's gate on every item the GPU test compares, and every such item
passes the conditioning probe; an all-zero reset table gives stretch_locked_roundtrip's bits; every mutant is seen by the case named for
it; the plan is non-decreasing, exactly hop apart inside spans, ends on base[nF - 1] and rejects an onset by each of its six conditions;
the pick on ties, plateaus, NaN, n = 1 and thr 0 and 1; the margin of every pick decision the GPU test relies on; vp_onset_pick and
vp_stretch_positions_transient equal NumPy exactly on a sweep, and the same sweep runs clean in a stand-alone program built with the address
and undefined-behaviour sanitizers; and the direction of the quality figures.  No GPU."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_stretch_lock_reference as SLR  # noqa: E402
import pv_transient_cases as TC  # noqa: E402
import pv_transient_reference as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = TC.F
VP_ERR_INVALID_ARG = -1


def _stage_items():
    return [it for c in TC.GPU_CASES for it in TC.gpu_items(c)] + TC.silent_items()


# ---- 1. the stage: two statements, the probe, the all-zero table ------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in TC.GPU_CASES if c.nF in (6, 19)], ids=TC.gpu_id)
def test_the_two_statements_agree_and_the_items_are_well_conditioned(c):
    for it in TC.gpu_items(c):
        gate, share = TC.gate_and_probe(it)
        print(f"PVTRANSIENT gate {it.name}: {gate:.3g}, probe {share:.3g} of the bound")
        assert gate <= TC.GATE_TOL, (it.name, gate)
        assert (share < TC.CONDITION_SHARE) == TC.pointwise(it), (it.name, share)


def test_the_small_and_the_silent_items_pass_gate_and_probe():
    items = [it for c in TC.GPU_CASES if c.nF in (1, 2, 5) for it in TC.gpu_items(c)] + TC.silent_items()
    for it in items:
        gate, share = TC.gate_and_probe(it)
        assert gate <= TC.GATE_TOL and (share < TC.CONDITION_SHARE) == TC.pointwise(it), (it.name, gate, share)
    assert len(TC.DEMOTED) <= 0.05 * len(_stage_items())


def test_silent_frames_are_where_the_silent_items_say_and_leave_theta():
    it = TC.silent_items()[0]
    w = TR.window(F)
    for f in range(TC.SILENT_NF):
        silent = not np.any(np.fft.rfft(it.x[it.pos[f]:it.pos[f] + F].astype(np.float64) * w))
        assert silent == (f in TC.SILENT_FRAMES), f
    assert it.reset[9] and it.reset[15] and 9 in TC.SILENT_FRAMES and 15 == TC.SILENT_FRAMES[-1] + 1
    # a flag on a silent frame changes nothing: the frame has no peak, theta stays
    only15 = it.reset.copy()
    only15[9] = 0
    a = TR.stretch_locked_reset_roundtrip(it.x, it.pos, it.T, it.ratio, it.reset, F, it.hop)
    assert np.array_equal(a, TR.stretch_locked_reset_roundtrip(it.x, it.pos, it.T, it.ratio, only15, F, it.hop))
    s3 = TC.silent_items()[3]
    assert np.array_equal(TC.reference(s3), SLR.stretch_locked_roundtrip(s3.x, s3.pos, s3.T, s3.ratio, F, s3.hop))


@pytest.mark.parametrize("hop", TC.HOPS)
def test_an_all_zero_table_gives_the_locked_stretch_bit_for_bit(hop):
    import pv_stretch_lock_cases as K
    for nF in (6, 19):
        c = next(g for g in K.GPU_CASES if g.hop == hop and g.nF == nF)
        for it in K.gpu_items(c):
            want = K.reference(it)
            for reset in (None, np.zeros(nF, np.uint8)):
                assert np.array_equal(TR.stretch_locked_reset_roundtrip(it.x, it.pos, it.T, it.ratio, reset, F, hop), want), it.name
            assert np.array_equal(TR.stretch_locked_reset_roundtrip_b(it.x, it.pos, it.T, it.ratio, np.zeros(nF, np.uint8), F, hop), K.reference(it, "b"))


def test_a_span_behind_a_reset_is_the_identity():
    """ratio 1 and frames hop apart from the flagged frame on: the stage returns the spectrum it was given, bit for bit."""
    pos, ratio, reset, n_in = TC.identity_tables(256, 1)
    x = TC.LC.voice(n_in, seed=5)
    st = TR.LR.LockState(F // 2 + 1)
    w = TR.window(F)
    q = TR.SR.clamp_positions(pos[0], n_in, F)
    D = TR.SR.advances(q, 256, F, "delta")
    for f in range(TC.IDENTITY_NF):
        X = np.fft.rfft(x[q[f]:q[f] + F].astype(np.float64) * w)
        Y = TR.reset_stage(X, ratio[0, f], int(D[f]), st, F, 256, bool(reset[0, f]))
        Xr = X.copy()
        Xr[0], Xr[-1] = X[0].real, X[-1].real
        assert np.array_equal(Y, Xr) == (f >= TC.IDENTITY_R), f


# ---- 2. teeth ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", TR.STAGE_MUTANTS)
def test_stage_mutants_are_seen(mutant):
    it = TC.teeth_stage_item(mutant)
    assert TC.pointwise(it)
    ref = TC.reference(it)
    dist = np.abs(TC.reference(it, mutant=mutant) - ref).max() / TC.bound(it.hop, ref)
    print(f"PVTRANSIENT teeth {mutant} on {it.name}: {dist:.3g} bounds")
    assert dist >= TC.TEETH, (mutant, dist)


@pytest.mark.parametrize("mutant", TR.FLUX_MUTANTS)
def test_flux_mutants_are_seen(mutant):
    _, name, hop = TC.TEETH_CASES[mutant]
    x = TC.row(name, TC.in_length(21, hop, 3), 3, hop)
    flux, _ = TR.onset_flux(x, F, hop)
    bad, _ = TR.onset_flux(x, F, hop, mutant)
    dist = np.abs(bad - flux)[1:-1] / TR.flux_bound(x, F, hop)[1:-1].clip(1e-300)
    print(f"PVTRANSIENT teeth {mutant}: {dist.max():.3g} bounds")
    assert dist.max() >= 1e6, (mutant, dist.max())


def test_pick_and_plan_mutants_are_seen():
    _, flux, mass = TC.TEETH_CASES["pick_ge"]
    assert list(TR.pick_onsets(flux, mass, 0.2)) == [0, 1, 0, 0, 0]
    assert list(TR.pick_onsets(flux, mass, 0.2, "pick_ge")) == [0, 1, 1, 0, 0]
    for mutant in TR.PLAN_MUTANTS:
        spec = TC.TEETH_CASES[mutant][1]
        why = []
        pos, reset = TC.plan_of(spec, why=why)
        bpos, breset = TC.plan_of(spec, mutant)
        assert why == ["accepted"] and reset.sum() == 1
        assert not (np.array_equal(pos, bpos) and np.array_equal(reset, breset)), mutant
    spec = TC.TEETH_CASES["fc_floor"][1]                       # (onset 15 at stretch 1.5)
    assert np.nonzero(TC.plan_of(spec)[1])[0][0] == 23 - spec["K"] and np.nonzero(TC.plan_of(spec, "fc_floor")[1])[0][0] == 22 - spec["K"]


# ---- 3. the plan -----------------------------------------------------------------------------------------------------------------------------------
def _check_plan(pos, reset, on, nF, hop, stretch, n_in, Kspan):
    assert pos.dtype == np.int32 and reset.dtype == np.uint8 and len(pos) == nF == len(reset)
    assert np.all(np.diff(pos.astype(np.int64)) >= 0) and pos[0] == 0
    base_last = min(int(np.floor(float((nF - 1) * hop) / stretch)), n_in - F)
    assert pos[-1] == base_last
    for a, b in TR.spans(reset, Kspan):
        assert np.all(np.diff(pos[a:b + 1].astype(np.int64)) == hop), (a, b)
        g = int(pos[a]) // hop + Kspan
        assert pos[a] % hop == 0 and on[g]


def test_the_plan_is_monotone_hop_apart_in_spans_and_ends_on_base():
    rng = np.random.default_rng(91)
    seen = 0
    for _ in range(300):
        hop = int(rng.choice(TC.HOPS))
        stretch = float(rng.choice([0.25, 0.5, 0.75, 1.0, 1.37, 1.5, 2.0, 4.0]))
        n_in = F + int(rng.integers(0, 80 * hop))
        nG = (n_in - F) // hop + 1
        nF = max(int(n_in * stretch - F) // hop + 1, 1)
        Kspan = int(rng.integers(1, 9))
        on = (rng.random(nG) < 0.08).astype(np.uint8)
        pos, reset = TR.plan_positions(on, nF, hop, stretch, n_in, F, Kspan)
        _check_plan(pos, reset, on, nF, hop, stretch, n_in, Kspan)
        seen += int(reset.sum())
    assert seen > 100


def test_without_an_accepted_onset_the_plan_is_the_two_anchor_line():
    nF, hop, stretch, n_in = 41, 256, 1.37, F + 30 * 256
    on = np.zeros((n_in - F) // hop + 1, np.uint8)
    pos, reset = TR.plan_positions(on, nF, hop, stretch, n_in, F, 2)
    last = min(int(np.floor((nF - 1) * hop / stretch)), n_in - F)
    assert not reset.any() and list(pos) == [(f * last) // (nF - 1) for f in range(nF)]
    base = np.minimum(np.floor(np.arange(nF) * hop / stretch), n_in - F)
    assert not np.array_equal(pos, base)                       # (the line, not vp_stretch_positions's table)
    assert list(TR.plan_positions(on[:1], 1, hop, 1.0, F, F, 2)[0]) == [0]


REJECTIONS = {
    # condition -> (nF, hop, stretch, n_in, K, onsets): the LAST onset listed is rejected by exactly this condition first
    "g-K": (60, 256, 1.0, F + 59 * 256, 2, (1,)),
    "g+K": (60, 256, 0.5, F + 59 * 256, 2, (58,)),
    "a": (60, 256, 1.0, F + 59 * 256, 2, (10, 13)),            # a = 11 is not behind the last anchor's frame 12
    "b": (30, 256, 1.0, F + 59 * 256, 2, (28,)),               # b = 30 is not in front of the last frame
    "pos-lo": (100, 256, 2.0, F + 59 * 256, 2, (10, 13)),      # frames 18 .. 22 and 24 .. 28, but the input spans 8 .. 12 and 11 .. 15 overlap
    "pos-hi": (60, 256, 4.0, F + 59 * 256, 2, (14,)),          # (g + K) hop = 4096 lies behind base[nF - 1] = 3776
}


@pytest.mark.parametrize("cond", list(REJECTIONS))
def test_an_onset_is_rejected_by_each_condition(cond):
    nF, hop, stretch, n_in, Kspan, onsets = REJECTIONS[cond]
    spec = dict(nF=nF, hop=hop, stretch=stretch, n_in=n_in, K=Kspan, onsets=onsets)
    why = []
    pos, reset = TC.plan_of(spec, why=why)
    assert why == ["accepted"] * (len(onsets) - 1) + [cond], why
    assert reset.sum() == len(onsets) - 1
    on = np.zeros((n_in - F) // hop + 1, np.uint8)
    on[list(onsets)] = 1
    _check_plan(pos, reset, on, nF, hop, stretch, n_in, Kspan)


def test_span_range_and_default():
    on = np.zeros(5, np.uint8)
    for bad in (0, 9):
        with pytest.raises(AssertionError):
            TR.plan_positions(on, 4, 256, 1.0, F + 4 * 256, F, bad)
    assert [TR.default_span(F, hop) for hop in (64, 128, 256, 512)] == [8, 4, 2, 1]


# ---- 4. the pick -----------------------------------------------------------------------------------------------------------------------------------
def test_pick_ties_plateaus_nan_and_the_thresholds():
    nan = float("nan")
    pick = lambda fl, ms, thr: list(TR.pick_onsets(np.array(fl, float), np.array(ms, float), thr))   # noqa: E731
    assert pick([3.0], [4.0], 0.5) == [1] and pick([0.0], [4.0], 0.0) == [0] and pick([], [], 0.5) == []      # n = 1: both neighbours missing
    assert pick([1.0, 1.0], [1.0, 1.0], 0.0) == [1, 0]                                   # a tie: its left end
    assert pick([0.0, 2.0, 2.0, 2.0, 1.0], [9.0] * 5, 0.1) == [0, 1, 0, 0, 0]            # a plateau: its left end
    assert pick([0.0, 1.0, 2.0, 3.0], [9.0] * 4, 0.0) == [0, 0, 0, 1]                    # a rise to the last frame
    assert pick([0.0, 2.0, nan, 2.0, 1.0, 3.0, 0.0], [9.0] * 7, 0.0) == [0, 0, 0, 0, 0, 1, 0]   # a NaN says no, and so do its neighbours
    assert pick([0.0, 2.0, 0.0], [9.0, nan, 9.0], 0.1) == [0, 0, 0] and pick([0.0, 2.0, 0.0], [9.0, nan, 9.0], 0.0) == [0, 0, 0]
    assert pick([0.0, 2.0, 0.0, 4.0, 0.0], [9.0, 2.0, 9.0, 4.5, 9.0], 1.0) == [0, 1, 0, 0, 0]   # thr 1: only a frame that is all rise
    assert pick([0.0, 2.0, 0.0, 4.0, 0.0], [9.0, 2.0, 9.0, 4.5, 9.0], 0.0) == [0, 1, 0, 1, 0]   # thr 0: every local maximum above 0
    for bad in (-0.1, 1.1):
        with pytest.raises(AssertionError):
            TR.pick_onsets(np.zeros(3), np.zeros(3), bad)


@pytest.mark.parametrize("c", TC.PICK_CASES, ids=lambda c: c.name)
def test_every_pick_decision_the_gpu_test_compares_has_a_wide_margin(c):
    x = TC.pick_input(c)
    flux, mass, _ = TC.flux_reference(x, c.hop, c.name)
    for s in range(len(x)):
        ok, smallest = TC.margins_ok(flux[s], mass[s])
        on = TR.pick_onsets(flux[s], mass[s], TC.THR)
        print(f"PVTRANSIENT margin {c.name} row {s}: smallest {smallest:.3g} of the mass, onsets {list(np.nonzero(on)[0])}")
        assert ok, (c.name, s, smallest)
        assert on.any()


# ---- 5. the library's host half against NumPy --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from vocoderproject_amd import load_library
    return load_library()


def _sweep(seed, n):
    """(nF, hop, stretch, n_in, K, onsets uint8 [nG]) x n: random onset sets, stretch 0.25 .. 4, hops 64 .. 512, every K, n_in down to F."""
    rng = np.random.default_rng(seed)
    for i in range(n):
        hop = int(rng.choice((64, 128, 256, 512)))
        stretch = float(rng.choice([0.25, 4.0, 1.0, rng.uniform(0.25, 4.0), rng.uniform(0.25, 4.0)]))
        n_in = F + (0 if i % 17 == 0 else int(rng.integers(0, 120 * hop)))
        nG = (n_in - F) // hop + 1
        nF = int(rng.integers(0, 3)) if i % 13 == 0 else max(int(n_in * stretch - F) // hop + 1 + int(rng.integers(-2, 3)), 0)
        on = (rng.random(nG) < rng.choice([0.0, 0.03, 0.1, 0.5, 1.0])).astype(np.uint8) * rng.integers(1, 256, nG).astype(np.uint8)
        yield nF, hop, stretch, n_in, 1 + i % 8, on


def test_the_library_plans_and_picks_exactly_as_numpy(lib):
    from vocoderproject_amd import pick_onsets, stretch_positions_transient, VpError
    spans = 0
    for nF, hop, stretch, n_in, Kspan, on in _sweep(92, 600):
        want_pos, want_reset = TR.plan_positions(on, nF, hop, stretch, n_in, F, Kspan)
        pos, reset = stretch_positions_transient(on, nF, hop, stretch, n_in, F, Kspan)
        assert np.array_equal(pos, want_pos) and np.array_equal(reset, want_reset), (nF, hop, stretch, n_in, Kspan)
        spans += int(reset.sum())
    assert spans > 300
    rng = np.random.default_rng(93)
    for i in range(300):
        n = int(rng.integers(0, 40))
        flux = np.round(rng.random(n) * 4) / 4 * rng.choice([0.0, 1.0, 1.0, 1.0], n)       # (ties and plateaus)
        mass = flux + rng.random(n) * rng.choice([0.0, 1.0, 5.0], n)
        if n and i % 3 == 0:
            (flux if i % 2 else mass)[rng.integers(0, n)] = np.nan
        thr = float(rng.choice([0.0, 1.0, 0.2, rng.random()]))
        assert np.array_equal(pick_onsets(flux, mass, thr), TR.pick_onsets(flux, mass, thr)), (flux, mass, thr)
    # the argument errors; nothing is written then
    pos, reset, on = np.full(4, 7, np.int32), np.full(4, 7, np.uint8), np.zeros(5, np.uint8)
    call = lib.vp_stretch_positions_transient
    good = [pos.ctypes.data, reset.ctypes.data, 4, 256, 1.0, F + 4 * 256, F, on.ctypes.data, 2]
    for i, bad in ((0, None), (1, None), (7, None), (2, -1), (3, 0), (4, 0.2), (4, 4.5), (4, float("nan")), (5, F - 1), (6, 0), (8, 0), (8, 9)):
        a = list(good)
        a[i] = bad
        assert call(*a) == VP_ERR_INVALID_ARG, (i, bad)
    assert np.all(pos == 7) and np.all(reset == 7)
    assert call(*good) == 0 and list(pos) == [0, 256, 512, 768] and not reset.any()
    fl, out = np.ones(3), np.full(3, 7, np.uint8)
    for a in ((None, fl.ctypes.data, 3, 0.2, out.ctypes.data), (fl.ctypes.data, None, 3, 0.2, out.ctypes.data), (fl.ctypes.data, fl.ctypes.data, 3, 0.2, None),
              (fl.ctypes.data, fl.ctypes.data, -1, 0.2, out.ctypes.data), (fl.ctypes.data, fl.ctypes.data, 3, 1.5, out.ctypes.data),
              (fl.ctypes.data, fl.ctypes.data, 3, -0.1, out.ctypes.data), (fl.ctypes.data, fl.ctypes.data, 3, float("nan"), out.ctypes.data)):
        assert lib.vp_onset_pick(*a) == VP_ERR_INVALID_ARG, a
    assert np.all(out == 7)
    assert lib.vp_onset_num_frames(F, F, 256) == 1 and lib.vp_onset_num_frames(F + 511, F, 256) == 2 and lib.vp_onset_num_frames(F - 1, F, 256) == VP_ERR_INVALID_ARG
    with pytest.raises(VpError):
        stretch_positions_transient(on, 4, 256, 1.0, F + 4 * 256, F, 9)
    with pytest.raises(ValueError):
        stretch_positions_transient(on[:3], 4, 256, 1.0, F + 4 * 256, F, 2)


def test_the_host_half_runs_clean_under_the_sanitizers(tmp_path):
    """tools/pv_transient_host_check.cpp compiles csrc/vp_onset_host.inc -- the text the library is built from -- into a stand-alone
    program with -fsanitize=address,undefined; the program reads the sweep's cases, writes the tables into exactly sized heap blocks and
    prints them, and they equal NumPy's."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = tmp_path / "host_check"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "vocoderproject_amd", "csrc"), os.path.join(ROOT, "tools", "pv_transient_host_check.cpp"), "-o", str(exe)])
    cases = list(_sweep(92, 200))
    lines = [f"{nF} {hop} {stretch!r} {n_in} {Kspan} " + "".join("1" if v else "0" for v in on) for nF, hop, stretch, n_in, Kspan, on in cases]
    rng = np.random.default_rng(94)
    picks = []
    for _ in range(100):
        n = int(rng.integers(1, 30))
        flux, mass = np.round(rng.random(n) * 4) / 4, rng.random(n) * 3
        picks.append((flux, mass, float(rng.choice([0.0, 0.2, 1.0]))))
        lines.append("pick " + f"{picks[-1][2]!r} " + " ".join(repr(float(v)) for v in np.concatenate((flux, mass))))
    run = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    out = run.stdout.strip().split("\n")
    assert len(out) == len(lines)
    for (nF, hop, stretch, n_in, Kspan, on), got in zip(cases, out):
        pos, reset = TR.plan_positions(on, nF, hop, stretch, n_in, F, Kspan)
        assert got.split() == ["0"] + [str(int(v)) for v in pos] + ["|"] + [str(int(v)) for v in reset], (nF, hop, stretch, n_in, Kspan)
    for (flux, mass, thr), got in zip(picks, out[len(cases):]):
        assert got.split() == ["0"] + [str(int(v)) for v in TR.pick_onsets(flux, mass, thr)]
    print(f"PVTRANSIENT sanitizers: {len(lines)} cases clean")


# ---- 6. what the scheme is for: direction only ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TC.QUALITY_CASES, ids=TC.quality_id)
def test_an_attack_stays_closer_to_the_input_than_under_the_locked_stretch(c):
    q = TC.quality(c, 0.0, n_onsets=2)
    assert any(r["accepted"] for r in q["rows"]), q
    for r in q["rows"]:
        print(f"PVTRANSIENT quality {TC.quality_id(c)} onset {r['onset']}: frame {r['frame']} accepted {r['accepted']}, distance {r['new']:.3g} (locked {r['old']:.3g}), "
              f"pre/post {r['new_pre']:.3g} (locked {r['old_pre']:.3g})")
        assert r["accepted"] and r["new"] < r["old"], (TC.quality_id(c), r)
