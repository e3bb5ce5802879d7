"""The peak-locked time stretch's EDGE cases on the CPU (tests/pv_stretch_lock_edge_cases.py; no GPU), as tests/test_pv_lock_edges_cpu.py has
them for the parent: the trace changes no bit of the definition; every case reaches the branch it names (predicates on the definition's
trace), passes the two-form gate and the lock family's conditioning probe -- no case is held to properties only; every branch of the list
is reached by a pointwise case that names it; what the 321 items of tests/test_gpu_pv_stretch_lock.py reach of the same branches is pinned
(the zeros are the gap these cases close); and every mutant of the definition -- the four of the first pass and the five edge mutants -- is
at least TEETH bounds away on a named case.  Run with -s for the STRETCHLOCKEDGE lines.

The probe is tests/test_pv_lock_edges_cpu.py's: every bin of every frame's spectrum moves by 1e-13 of the frame's largest magnitude, bins 0
and N along the real axis only (the transform of a real frame leaves them real in NumPy and in the kernel, so the exact ties of the unwrap
there are the definition's rule, not a matter of conditioning); the output must move by less than 1 % of the case's GPU bound, on three
seeds.

The tie the copy adds to the parent's: with an odd advance D the nominal term (N D) / F of bin N is a half-integer, so two frames whose
bin-N phases are EQUAL give d = -1/2 exactly, and rint's half-to-even rule decides between nu = N - F / (2 D) and N + F / (2 D).  Measured
on tieN-freeze (D = 1, -5 semitones), the definition with the half rounded away from zero is 1.83e4 (hop 64), 4.84e5 (hop 256) and 1.54e6
(hop 512) bounds away.  All 41 cases pass gate (worst 1.24e-13, gone-hop512) and probe (worst 6.4e-5 of the bound, slot1-leap-one-hop512)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_lock_cases as LC  # noqa: E402
import pv_stretch_lock_cases as K  # noqa: E402
import pv_stretch_lock_edge_cases as SE  # noqa: E402
import pv_stretch_lock_reference as SLR  # noqa: E402

F, N = LC.F, LC.F // 2
CONDITION_EPS, CONDITION_SEEDS, CONDITION_SHARE = K.CONDITION_EPS, K.CONDITION_SEEDS, K.CONDITION_SHARE
assert (CONDITION_EPS, CONDITION_SEEDS, CONDITION_SHARE) == (1e-13, (0, 1, 2), 0.01)

# cases that miss the gate or the conditioning probe would be held to properties only: none may be (a case that misses is replaced)
PROPERTIES_ONLY = ()
POINTWISE = [c for c in SE.CASES if c.name not in PROPERTIES_ONLY]
TRACE_KEYS = {"P", "own", "Ps", "Pa", "owns", "r", "silent", "gone", "tie", "q", "D"}


# ---- 1. the trace changes no bit ---------------------------------------------------------------------------------------------------------------
def test_the_trace_changes_no_bit_of_the_384_gate_cases():
    import pv_stretch_reference as SR
    assert len(K.GATE_CASES) == 384
    for c in K.GATE_CASES:
        it, tr = K.gate_item(c), []
        y = SLR.stretch_locked_roundtrip(it.x, it.pos, it.T, it.ratio, F, it.hop, trace=tr)
        assert np.array_equal(y, K.reference(it)), it.name
        assert len(tr) == c.nF and all(set(t) == TRACE_KEYS for t in tr)
        q = SR.clamp_positions(it.pos, len(it.x), F)
        assert [t["q"] for t in tr] == list(q) and [t["D"] for t in tr] == list(SR.advances(q, it.hop, F))


# ---- 2. gate, conditioning, predicates -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SE.CASES, ids=lambda c: c.name)
def test_every_case_passes_the_gate_is_well_conditioned_and_reaches_its_branch(c):
    y, tr = SE.reference(c)
    yb, _ = SE.reference(c, "b")
    gate = np.abs(y - yb).max() / max(1.0, float(np.abs(y).max()))
    bnd = LC.bound(c.hop, y)
    x, pos, r, T = SE.burst_input(c), SE.case_positions(c), SE.case_ratios(c), SE.length(c)
    moved = max(np.abs(SLR.stretch_locked_roundtrip(x, pos, T, r, F, c.hop, perturb=(CONDITION_EPS, s)) - y).max() for s in CONDITION_SEEDS)
    print(f"STRETCHLOCKEDGE cpu {c.name}: gate {gate:.3g} moved {moved / bnd:.3g} of the bound, max |ref| {np.abs(y).max():.3g}")
    assert T == F + (c.nF - 1) * c.hop + 3 and len(tr) == c.nF and all(set(t) == TRACE_KEYS for t in tr)
    assert np.abs(y).max() > 100.0 * bnd or all(t["silent"] or t["gone"] for t in tr), c.name            # the comparison is not vacuous
    assert c.name not in PROPERTIES_ONLY
    assert gate <= LC.GATE_TOL, (c.name, gate)
    assert moved < CONDITION_SHARE * bnd, (c.name, moved, bnd)
    for pred, arg in c.expect:
        n = SE.count(c, pred, arg)
        print(f"STRETCHLOCKEDGE cpu {c.name}: {pred}({arg}) on {n} frames")
        assert n >= 1, (c.name, pred, arg)


def test_every_required_branch_is_reached_by_a_pointwise_case():
    assert PROPERTIES_ONLY == () and len(POINTWISE) == len(SE.CASES)
    assert len(SE.GROUPS) <= 12 and all(len(v) <= 8 for v in SE.GROUPS.values())
    assert {c.hop for c in SE.CASES} == {64, 256, 512} and all(c.nF <= 16 for c in SE.CASES)
    assert any(c.n_in % 2 == 1 for c in SE.CASES) and any(c.n_in % 2 == 0 for c in SE.CASES)
    assert any(min(c.pos) < 0 for c in SE.CASES) and any(max(c.pos) > c.n_in - F for c in SE.CASES)
    for pred, arg in SE.REQUIRED:
        n = {c.name: SE.count(c, pred, arg) for c in POINTWISE}
        total = sum(n.values())
        print(f"STRETCHLOCKEDGE reach {pred}({arg}): {total} frames in {sum(v > 0 for v in n.values())} cases")
        assert total >= 1, (pred, arg)
        assert any(n[c.name] > 0 and (pred, arg) in c.expect for c in POINTWISE), (pred, arg)              # and a case names it
    # at hop 64 and at hop 512 at least
    for hop in (64, 512):
        for pred, arg in SE.REQUIRED:
            assert any(c.hop == hop and (pred, arg) in c.expect for c in POINTWISE), (hop, pred, arg)


def test_the_zero_rotation_factor_leaves_the_region_unturned():
    """r hop == D at D != hop: the peak's angle is the one it had (theta of frame 0 is 0 here, so the frame's spectrum is only shifted)."""
    for name in ("turn-hop64", "turn-hop256", "turn-hop512"):
        c = SE.BY_NAME[name]
        tr = SE.reference(c)[1]
        f = next(f for f, t in enumerate(tr) if SE._sounding(t) and t["r"] * c.hop == t["D"] and t["D"] != c.hop)
        assert f == 1 and tr[1]["D"] == 3 * c.hop // 4
        # frame 1 alone, behind frame 0: theta after frame 0 is nu (0.75 hop - hop) / F; frame 1 adds exactly nothing to it
        x, pos, r = SE.burst_input(c), SE.case_positions(c), SE.case_ratios(c)
        st = SLR.LR.LockState(N + 1)
        w = SLR.window(F)
        q = SLR.SR.clamp_positions(pos, c.n_in, F)
        SLR.stretch_lock_stage(np.fft.rfft(x[q[0]:q[0] + F].astype(np.float64) * w), 0.75, c.hop, st, F, c.hop)
        before = st.theta.copy()
        SLR.stretch_lock_stage(np.fft.rfft(x[q[1]:q[1] + F].astype(np.float64) * w), 0.75, tr[1]["D"], st, F, c.hop)
        P = tr[1]["P"]
        assert np.array_equal(st.theta[P], before[P] - np.rint(before[P])), name


# ---- 3. what the first pass's 321 GPU items reach: pinned ------------------------------------------------------------------------------------------
def _gpu_file_items():
    items = [it for c in K.GPU_CASES for it in K.gpu_items(c)] + [it for c in K.EDGE_CASES for it in K.edge_case_items(c)]
    items += [it for c, n_in in K.SMALL_CASES for it in K.edge_case_items(c, n_in)] + K.big_items()
    return items


def test_what_the_first_pass_reaches_is_pinned():
    items = _gpu_file_items()
    traces = []
    for it in items:
        tr = []
        SLR.stretch_locked_roundtrip(it.x, it.pos, it.T, it.ratio, F, it.hop, trace=tr)
        traces.append(tr)
    frames = [t for tr in traces for t in tr]
    got = {k: sum(SE.PREDICATES[k](None, tr, None) for tr in traces) for k in ("any_silent", "any_gone", "behind_silent_any", "single_peak")}
    lowest = max(int(t["P"][0]) for t in frames if len(t["P"]))
    ties = sum(N in t["tie"] and t["D"] % 2 == 1 for tr in traces for t in tr[1:])
    print(f"STRETCHLOCKEDGE first pass: {len(items)} items, {len(frames)} frames, {got}, largest lowest peak {lowest}, bin-N ties at an odd D {ties}")
    assert len(items) == 321 and len(frames) == 2699
    assert got == {"any_silent": 0, "any_gone": 0, "behind_silent_any": 0, "single_peak": 5}, got
    assert lowest == 13, lowest


# ---- 4. teeth ----------------------------------------------------------------------------------------------------------------------------------------
TEETH_CASES = {
    "hop": "slot3-reverse-above-hop512", "nod": "turn-hop512", "late": "gone-hop512", "nohigh": "slot3-reverse-above-hop64",
    "silent_theta": "slot1-leap-one-hop512", "silent_prev": "slot1-leap-one-hop512", "tie_away": "tieN-freeze-hop64", "drop_n": "edge15-hop512",
    "hop_after_silent": "slot0-low-odd-1000-hop512",
}


@pytest.mark.parametrize("mutant", SLR.MUTANTS + SLR.EDGE_MUTANTS)
def test_every_mutant_is_seen_by_a_named_edge_case(mutant):
    assert set(TEETH_CASES) == set(SLR.MUTANTS + SLR.EDGE_MUTANTS) and all(v not in PROPERTIES_ONLY for v in TEETH_CASES.values())
    c = SE.BY_NAME[TEETH_CASES[mutant]]
    y = SE.reference(c)[0]
    away = np.abs(SE.reference(c, "a", mutant)[0] - y).max() / LC.bound(c.hop, y)
    seen = [k.name for k in POINTWISE if np.abs(SE.reference(k, "a", mutant)[0] - SE.reference(k)[0]).max() > LC.bound(k.hop, SE.reference(k)[0])]
    print(f"STRETCHLOCKEDGE mutant {mutant}: {away:.3g} bounds away on {c.name}; changes {len(seen)} of {len(POINTWISE)} edge cases")
    assert away >= LC.TEETH, (mutant, away)


@pytest.mark.parametrize("hop", [64, 256, 512])
def test_the_tie_rule_shows_at_every_hop(hop):
    c = SE.BY_NAME[f"tieN-freeze-hop{hop}"]
    y = SE.reference(c)[0]
    away = np.abs(SE.reference(c, "a", "tie_away")[0] - y).max() / LC.bound(hop, y)
    print(f"STRETCHLOCKEDGE mutant tie_away: {away:.3g} bounds away on {c.name}")
    assert SE.count(c, "tie_n_same_sign", None) >= 1 and away >= LC.TEETH, (hop, away)


def test_the_edge_mutants_leave_the_first_pass_alone():
    """The mutants that need a silent frame change no item of the first pass (it has none); the tie rule and the dropped peak do."""
    items = _gpu_file_items()
    for mutant in ("silent_theta", "silent_prev", "hop_after_silent"):
        for it in items[::7]:
            assert np.array_equal(SLR.stretch_locked_roundtrip(it.x, it.pos, it.T, it.ratio, F, it.hop, mutant), K.reference(it)), (mutant, it.name)
