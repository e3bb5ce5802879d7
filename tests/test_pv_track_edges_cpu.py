"""CPU-side checks of the pitch trackers' EDGE cases (tests/pv_track_edge_cases.py), which tests/test_gpu_pv_track_edges.py compares with
the kernels bit for bit: the walk and the note lookup written out in Python (pv_track_reference.walk, closest) equal the oracle's yin_pick
and notes_closest on every frame of the first table and of the edge table; every edge case reaches the branch it exists for; the first
table's blind spots are what they were found to be; every new seeded fault changes the definition on a named edge case, and the number of
first-table cases it changes is asserted; the conditioning bounds of the first table hold on the edge cases.  One line per finding is
printed (-s).

Figures (printed by the tests below, asserted where they are stated as equalities):
  first table       90 cases, 2805 frames, 2136 voiced: 0 frames with idx == notesN, 0 with first == tau0, 17 with first == tauMax - 1 and
                    none of those with ks == first, 28 with ks == first, 4 with first % 64 == 63;
  edge table        74 cases, 939 frames, 894 voiced: 193 frames with idx == notesN, 195 with first == tau0, 114 with
                    first == tauMax - 1, all of them with ks == first, 587 with ks == first, 155 with first % 64 == 63, 165 with
                    first % 64 == 0;
  faults            first-table cases changed (of 90) / edge cases changed (of 74): popped_zero 0 / 10, popped_clamped 0 / 10,
                    tau0_exclusive 0 / 11, last_lag_always_next 0 / 32, word_edge 5 / 26, owners_floor 27 / 25 (the first table's
                    tauMax = 441 has one lag in its partial owner lane, and its 100.2 Hz and 90 Hz rows end on it); streaming, in the mixed
                    grouping, first-table cases changed (of 8) / edge cases changed (of the 7 with N > 1): ring_phase 5 / 7, carry_gt 3 / 7.
Runtime: 12 s for the file on the development machine's CPU (budget: a minute)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_track_cases as TC  # noqa: E402
import pv_track_edge_cases as EC  # noqa: E402
import pv_track_reference as R  # noqa: E402
import pv_track_stream_cases as SC  # noqa: E402
import pv_track_stream_reference as SR  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the first table, once: its functions, the oracle's decisions and the Python walk's ---------------------------------------------------------
_OLD = {}


def _old(c):
    """(period, ratio, function, detail) of a first-table case from walk() and closest()."""
    if c not in _OLD:
        d = {}
        p, r, fn = R.track(TC.case_input(c), c.fs, c.F, c.hop, c.keys, with_function=True, detail=d)
        d["tau"] = p
        _OLD[c] = (p, r, fn, d)
    return _OLD[c]


def _census(details_and_fs):
    """Frames per branch over (detail, fs) pairs."""
    n = dict(frames=0, voiced=0, popped=0, first_tau0=0, last_lag=0, last_lag_stays=0, ks_first=0, word_end=0, word_start=0)
    for d, fs in details_and_fs:
        t0, tm = R.tau_min(fs), R.tau_max(fs)
        v = d["tau"] > 0
        n["frames"] += v.size
        n["voiced"] += int(v.sum())
        n["popped"] += int((v & (d["idx"] == d["notesN"])).sum())
        n["first_tau0"] += int((d["first"] == t0).sum())
        n["last_lag"] += int((d["first"] == tm - 1).sum())
        n["last_lag_stays"] += int(((d["first"] == tm - 1) & (d["ks"] == d["first"])).sum())
        n["ks_first"] += int((v & (d["ks"] == d["first"])).sum())
        n["word_end"] += int((v & (d["first"] % 64 == 63)).sum())
        n["word_start"] += int((v & (d["first"] % 64 == 0)).sum())
    return n


def test_python_walk_and_lookup_equal_the_oracle_on_every_old_and_new_case():
    for c in TC.CASES:
        p, r, _, _ = _old(c)
        want_p, want_r = TC.reference(c)
        assert np.array_equal(p, want_p) and np.array_equal(_bits(r), _bits(want_r)), TC.case_id(c)
    for c in EC.CASES:
        p, r, _ = EC.reference(c)
        want_p, want_r = R.track(EC.batch_input(c), c.fs, c.F, c.hop, c.keys)               # the oracle's yin_pick and notes_closest
        assert np.array_equal(p, want_p) and np.array_equal(_bits(r), _bits(want_r)), c.name


def test_first_table_blind_spots_are_as_found():
    n = _census((_old(c)[3], c.fs) for c in TC.CASES)
    print(f"PV TRACK EDGES first table: {len(TC.CASES)} cases {n}")
    assert (len(TC.CASES), n["frames"], n["voiced"]) == (90, 2805, 2136)
    assert n["popped"] == 0 and n["first_tau0"] == 0 and n["last_lag_stays"] == 0
    assert n["last_lag"] == 17 and n["ks_first"] == 28 and n["word_end"] == 4
    assert {R.tau_max(c.fs) for c in TC.CASES} == {441, 480, 80, 512}
    assert {(64 // c.N, 64 % c.N) for c in SC.CASES} == {(1, 0), (0, 64)}


# ---- every case reaches its branch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", EC.CASES, ids=EC.case_id)
def test_case_reaches_its_branch_and_is_conditioned(c):
    p, r, d = EC.reference(c)
    nF = R.n_frames(EC.length(c), c.F, c.hop)
    assert p.shape == r.shape == (EC.N_STREAMS, nF) and (c.length != "min" or EC.length(c) == c.F + R.tau_max(c.fs))
    for s in range(EC.N_STREAMS):
        assert EC.holds(c, s), (c.name, s, c.expect[s], d["first"][s].tolist(), d["ks"][s].tolist(), p[s].tolist(), d["idx"][s].tolist())
    # the first table's conditioning bounds
    assert np.all((r >= 0.5) & (r <= 2.0)) and np.all(r[p == 0] == 1.0)
    assert np.all((p == 0) | ((p >= R.tau_min(c.fs)) & (p <= R.tau_max(c.fs))))


def test_edge_table_census():
    n = _census((EC.reference(c)[2], c.fs) for c in EC.CASES)
    print(f"PV TRACK EDGES edge table: {len(EC.CASES)} cases {n}")
    assert n["popped"] > 0 and n["first_tau0"] > 0 and n["last_lag_stays"] > 0 and n["word_end"] > 0 and n["word_start"] > 0
    for lo in range(64, 512, 64):                                                    # first at both sides of every ballot word
        firsts = {int(v) for c in EC.TILED_CASES for v in EC.reference(c)[2]["first"].ravel()}
        assert {lo - 1, lo} <= firsts, lo
    for tm in EC.RESIDUE_TAUMAX:                                                     # ... and of the walk's last lag, at every residue
        for ln in ("clamp", "min"):
            d = EC.reference(EC.BY_NAME[f"residue-tm{tm}-{ln}"])[2]
            assert np.all(d["first"][0] == tm - 1) and np.all(d["ks"][0] == tm - 1) and np.all(d["tau"][0] == tm - 1)
            assert np.any((d["tau"][1] == tm - 1) & (d["first"][1] < tm - 1))        # sine_edge: the other side, tau = first + ... capped


def test_top_cases_read_and_return_the_popped_slot():
    """idx == notesN in every key; in the scale keys (top note 739.99 Hz, popped slot 830.6 Hz) the popped slot is the nearer one
    for periods up to tau0 + 1, and the ratio is popped / pitch > 1; for longer periods, and in the chromatic table (top note 783.99 Hz)
    at every period, the popped slot is compared and the top note returned (ratio < 1)."""
    returned = compared = 0
    for c in EC.TOP_CASES:
        p, r, d = EC.reference(c)
        for s, key in enumerate(c.keys):
            f, n = R.notes_table(key)
            popped = (d["idx"][s] == n)
            assert n == d["notesN"][s, 0] and f[n] > f[n - 1] > 0.0
            if c.expect[s][0].startswith("all_popped"):
                assert np.all(popped)
                pitch = c.fs / p[s].astype(np.float64)
                if np.all(pitch > 0.5 * (f[n] + f[n - 1])):                        # nearer to the popped slot: it is returned
                    assert key != 12 and np.all(r[s] > 1.0) and np.array_equal(_bits(r[s]), _bits(f[n] / pitch)), (c.name, s)
                    returned += 1
                else:                                                              # ... or only compared: the top note is returned
                    assert np.all(pitch < 0.5 * (f[n] + f[n - 1])) and np.all(r[s] < 1.0), (c.name, s)
                    assert np.array_equal(_bits(r[s]), _bits(f[n - 1] / pitch)), (c.name, s)
                    compared += 1
    print(f"PV TRACK EDGES top: streams whose frames return the popped slot {returned}, only compare it {compared}")
    assert (returned, compared) == (12, 18)
    assert any(c.expect[0][0] == "all_popped_first_tau0" for c in EC.TOP_CASES)
    p, _, d = EC.reference(EC.BOTTOM_CASE)
    assert np.all(d["idx"] == 0) and np.all(p == R.tau_max(EC.BOTTOM_CASE.fs) - 1)


def test_amplitude_twins_agree():
    c = EC.BY_NAME["degenerate-twins"]
    x = EC.batch_input(c)
    assert np.abs(x[1]).max() > 1e17 and 0.0 < np.abs(x[2]).max() < 1e-18
    p, r, _ = EC.reference(c)
    assert np.all(p[0] > 0) and np.array_equal(p[1], p[0]) and np.array_equal(p[2], p[0])
    assert np.array_equal(_bits(r[1]), _bits(r[0])) and np.array_equal(_bits(r[2]), _bits(r[0]))


def test_many_stream_batch_leaves_a_partial_workgroup():
    x, keys, p, r = EC.many_input()
    nF = p.shape[1]
    assert x.shape[0] == EC.MANY_S == len(keys) and (EC.MANY_S * nF) % EC.VP_TRACK_WAVES != 0 and ((EC.MANY_S + 1) * nF) % EC.VP_TRACK_WAVES == 0
    assert len({c for c, _ in EC.many_rows()}) == len(EC.MANY_SOURCES) >= 10 and len(set(keys)) >= 3
    assert np.any(p == 0) and np.any(p > 0)


# ---- teeth: the batch faults ------------------------------------------------------------------------------------------------------------------------
def _old_cases_changed(mutant):
    hits = []
    for c in TC.CASES:
        p, r, fn, _ = _old(c)
        if mutant == "owners_floor":
            if R.tau_max(c.fs) % 8 == 0:
                continue                                                             # (every owner lane is whole: the fault has no lag to act on)
            pm, rm = R.track(TC.case_input(c), c.fs, c.F, c.hop, c.keys, mutant=mutant)
        else:
            tm = R.tau_max(c.fs)
            got = [[R.decide(fn[s, f], tm, c.fs, R.norm_key(c.keys[s]), mutant) for f in range(p.shape[1])] for s in range(p.shape[0])]
            pm = np.array([[g[2] for g in row] for row in got], np.int32)
            rm = np.array([[g[4] for g in row] for row in got], np.float64)
        if not (np.array_equal(p, pm) and np.array_equal(_bits(r), _bits(rm))):
            hits.append(TC.case_id(c))
    return hits


# fault -> (what it must change, the edge case it must change it on, first-table cases it changes)
TEETH = {
    "popped_zero": ("ratio", "top-fs44100-F1024-p55", 0),
    "popped_clamped": ("ratio", "top-fs48000-F2048-p61", 0),
    "tau0_exclusive": ("period", "top-fs44100-F1024-p55", 0),
    "last_lag_always_next": ("period", "residue-tm445-min", 0),
    "word_edge": ("period", "tiled-fs51200-F2048-P127_128_191", 5),
    "owners_floor": ("period", "residue-tm447-clamp", 27),
}
assert set(TEETH) == set(R.EDGE_MUTANTS)


@pytest.mark.parametrize("mutant", sorted(TEETH))
def test_seeded_fault_changes_the_definition_on_a_named_edge_case(mutant):
    what, name, old_hits = TEETH[mutant]
    c = EC.BY_NAME[name]
    p, r, _ = EC.reference(c)
    pm, rm = R.track(EC.batch_input(c), c.fs, c.F, c.hop, c.keys, mutant=mutant)
    if what == "period":
        assert not np.array_equal(p, pm), (mutant, name)
    else:
        assert np.array_equal(p, pm) and not np.array_equal(_bits(r), _bits(rm)), (mutant, name)
    changed = []
    for e in EC.CASES:
        ep, er, _ = EC.reference(e)
        em_p, em_r = R.track(EC.batch_input(e), e.fs, e.F, e.hop, e.keys, mutant=mutant)
        if not (np.array_equal(ep, em_p) and np.array_equal(_bits(er), _bits(em_r))):
            changed.append(e.name)
    hits = _old_cases_changed(mutant)
    print(f"PV TRACK EDGES fault {mutant}: first-table cases changed {len(hits)} {hits[:3]}; edge cases changed {len(changed)} {changed[:4]}")
    assert name in changed
    assert len(hits) == old_hits, (mutant, len(hits), hits)


# ---- streaming -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", EC.STREAM_CASES, ids=SC.case_id)
def test_stream_case_is_conditioned_and_its_silent_tails_have_their_length(c):
    x = EC.stream_input(c)
    p, r, raw = EC.stream_reference(c)
    fd = SC.first_decision(c)
    assert c.n_blocks == fd + EC.EXTRA_BLOCKS and x.shape == (c.n_blocks, len(c.signals), c.N)
    assert np.all(p[:fd] == 0) and np.all(r[:fd] == 1.0) and np.all((r >= 0.5) & (r <= 2.0))
    tm, t0 = R.tau_max(c.fs), R.tau_min(c.fs)
    for s, sp in enumerate(c.signals):
        if sp == ("tiled", tm - 1):
            assert np.all(p[fd:, s] == tm - 1)
        elif sp[0] == "tiled":
            assert np.all(p[fd:, s] == sp[1])
        elif sp[0] == "sine_p":
            assert np.all(p[fd:, s] == t0)                                          # the top of the range: the popped slot
    for s, run in EC.gap_streams(c):
        tail = p[fd:, s]
        assert run in (c.hold, c.hold + 1) and np.all(tail[:len(tail) - run] > 0) and np.all(tail[len(tail) - run:] == 0), (s, run, tail)
        # a run of `hold` blocks keeps the target, one of hold + 1 lets it go: the last block moves towards 1.0 by the glide
        if run > c.hold:
            before = r[-2, s]
            assert r[-1, s] == (1.0 if c.glide == 1.0 else before + c.glide * (1.0 - before)), (s, r[-3:, s])
        else:
            assert r[-1, s] != 1.0
    if c.N > 1:
        assert {run - c.hold for _, run in EC.gap_streams(c)} == ({1} if c.hold == 0 else {0, 1})
    # the groupings do not enter the definition
    for name, groups in EC.stream_groupings(c).items():
        if name in ("mixed", "below-W") and c.N > 1:
            gp, gr = SR.run(x, c.fs, c.F, c.keys, c.hold, c.glide, groups)
            assert np.array_equal(gp, p) and np.array_equal(_bits(gr), _bits(r)), name


def _stream_changed(cases, mutant, inp, ref, groupings):
    hits = []
    for c in cases:
        x = inp(c)
        p, r = ref(c)[:2]
        pm, rm = SR.run(x, c.fs, c.F, c.keys, c.hold, c.glide, groupings(c)["mixed"], mutant=mutant)
        if not (np.array_equal(p, pm) and np.array_equal(_bits(r), _bits(rm))):
            hits.append(c.name)
    return hits


# fault -> (the edge case it must change, first-table cases it changes in the mixed grouping)
STREAM_TEETH = {"ring_phase": ("edge-fs44100-F1024-n24-hold1", 5), "carry_gt": ("edge-fs44100-F1024-n63-hold0", 3)}
assert set(STREAM_TEETH) == set(SR.GATHER_MUTANTS)


@pytest.mark.parametrize("mutant", sorted(STREAM_TEETH))
def test_gather_fault_changes_the_definition_on_a_named_edge_case(mutant):
    name, old_hits = STREAM_TEETH[mutant]
    new = _stream_changed([c for c in EC.STREAM_CASES if c.N > 1], mutant, EC.stream_input, EC.stream_reference, EC.stream_groupings)
    old = _stream_changed(SC.CASES, mutant, SC.case_input, SC.reference, SC.groupings)
    print(f"PV TRACK EDGES gather fault {mutant} (mixed grouping): first-table cases changed {len(old)} {old}; edge cases changed {len(new)} {new}")
    assert name in new
    assert len(old) == old_hits, (mutant, old)
    if mutant == "carry_gt":
        assert "n64" not in old                                                      # r64 = 0: the carry is never taken late
