"""The pitch trackers' EDGE cases: inputs that take the branches of csrc/vp_track_body.inc and of the streaming gather which the first
case tables (tests/pv_track_cases.py, tests/pv_track_stream_cases.py) stay away from.  tests/test_pv_track_edges_cpu.py asserts, on the
definition, that every case reaches the branch it exists for; tests/test_gpu_pv_track_edges.py compares the kernels with the definition
bit for bit on the same cases.  Test infrastructure only.  Three streams per batch case, seeded, no float32 denormal and no non-finite
sample (batch_input and stream_input assert both).

A batch case names its branch as `expect`: one entry per stream, a predicate on that stream's frames of the definition's
(first, ks, tau, idx, notesN) -- see PREDICATES.  A case that does not reach its branch fails the CPU file.

  top        sines of period tau0 .. tau0 + 4 samples, keys (12, 0, 7): the pitch lies above the key's top note, lower_bound returns
             notesN and the popped slot behind the table is read (and, in the scale keys, returned); first == tau0 on the first of them;
  bottom     a pitch below the table's first entry (idx == 0): the other end of the lookup;
  tiled      a float32 noise pattern of P samples tiled along the row: d[P] == 0 exactly, so first == ks == tau == P for every P in
             [tau0, tauMax - 1] -- both sides of every ballot word, the `tau = first` side of the walk's last lag, exact zeros in d;
             P = tau0 - 1 gives 2 P (the lag under the tolerance below tau0 is ignored), P = tauMax is unvoiced;
  residue    fs = 100 tauMax for tauMax at every residue mod 8 and at both sides of a ballot word: the partial last owner lane of the
             normalisation carry and the `k >= tauMax` zeroing, on rows of the "clamp" length and of T = F + tauMax;
  degenerate DC (0 * inf = NaN: unvoiced), DC then tone, 700 zeros then tone, one impulse, alternating +-1, a voiced row with its 1e18 and
             2^-60 twins, -0.0 silence;
  many       MANY_S streams: the rows of the 44100 / 1024 / 256 cases above, in a batch whose frame count is no multiple of the
             kernel's frames per workgroup.

The long descent (a descent from `first` that stops two or more ballot words behind it) is NOT here: long_descent_search() found
none.  Searched at fs 51200 (tauMax 512, F 1024 and 2048; 100000 seeded candidates, 70 s of CPU): sines and mixtures of two and three
harmonics with a fundamental period of 0.8 .. 2.0 tauMax, a third of them chirped by up to +-20 % along the row, under flat, exponential
(rising and falling), linear and raised-cosine amplitude envelopes.  The longest descent found crosses ONE word boundary (period 410.3,
second harmonic 0.12, falling exponential: first 362, stop 409): 47 lags.  A sine of period T is under the tolerance only within about
0.12 T of T and the walk starts at 511 at the latest, so two boundaries (65 lags at least) need T >= 540, whose dip begins behind lag 470.
The descent's masks are reached one word at a time by the tiled cases (first at both sides of every word) and the "sine_edge" rows.

The streaming cases are tests/pv_track_stream_cases.py StreamCases whose `signals` are the specs of this file: every block size whose
gather steps (q64, r64) = (64 / N, 64 % N) the first table does not take -- N = 1 (64, 0), 24 (2, 16), 48 (1, 16), 63 (1, 1), 65 (0, 64),
100 (0, 64) -- fed with the tiled and top-of-range signals, and streams that fall silent so that the unvoiced run at the end of the
case is exactly `hold` and exactly `hold + 1` blocks long."""
from collections import namedtuple

import numpy as np

import pv_track_cases as TC
import pv_track_reference as R
import pv_track_stream_cases as SC
import pv_track_stream_reference as SR

N_STREAMS = 3
VP_TRACK_WAVES = 4          # csrc/vp_track.h: frames per workgroup
MANY_S = 299                # 300 rows of 5 frames would fill 375 workgroups exactly; 299 leave the last one three frames

EdgeCase = namedtuple("EdgeCase", "name fs F hop length signals keys expect")


# ---- signals ----------------------------------------------------------------------------------------------------------------------------------
def edge_signal(spec, n, fs, seed):
    """float32 [n].  A spec is a tuple: its first entry names the signal."""
    kind = spec[0]
    t = np.arange(n) / fs
    if kind == "tc":                                                               # a signal of the first table
        return TC.signal(spec[1], n, fs, seed).astype(np.float32)
    if kind == "tiled":                                                            # float32 noise of spec[1] samples, repeated
        pat = (0.5 * np.random.default_rng([seed, spec[1], 77]).standard_normal(spec[1])).astype(np.float32)
        return np.tile(pat, n // spec[1] + 1)[:n]
    if kind == "sine_p":                                                           # 0.8 sin with a period of spec[1] samples
        return (0.8 * np.sin(2.0 * np.pi * np.arange(n) / spec[1] + 0.3)).astype(np.float32)
    if kind == "dc":
        return np.full(n, spec[1], np.float32)
    if kind == "dc_tone":                                                          # DC over what frame 0 reads, then 220 Hz
        y = 0.8 * np.sin(2.0 * np.pi * 220.0 * t + 0.3)
        y[:spec[1]] = 0.5
        return y.astype(np.float32)
    if kind == "zeros_tone":
        y = 0.8 * np.sin(2.0 * np.pi * 220.0 * t + 0.3)
        y[:spec[1]] = 0.0
        return y.astype(np.float32)
    if kind == "tone_zeros":                                                       # 196 Hz, silent from sample spec[1] on
        y = 0.7 * np.sin(2.0 * np.pi * 196.0 * t + 0.2)
        y[spec[1]:] = 0.0
        return y.astype(np.float32)
    if kind == "impulse":
        y = np.zeros(n, np.float32)
        y[spec[1]] = 1.0
        return y
    if kind == "alt":
        return np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)
    if kind == "scaled":                                                           # spec[1] times the float32 row of spec[2]
        return (edge_signal(spec[2], n, fs, seed) * np.float32(spec[1])).astype(np.float32)
    if kind == "negzero":
        return np.full(n, -0.0, np.float32)
    raise KeyError(spec)


def make_rows(specs, n, fs, seed):
    x = np.stack([edge_signal(sp, n, fs, seed) for sp in specs])
    assert x.dtype == np.float32 and TC.no_denormals(x) and np.all(np.isfinite(x)), specs
    return x


# ---- predicates on one stream's frames ------------------------------------------------------------------------------------------------------------
# d: the tables first, ks, tau, idx, notesN of the stream, int [nF]; arg: the predicate's parameter
PREDICATES = {
    "all_at": lambda d, P: np.all((d["first"] == P) & (d["ks"] == P) & (d["tau"] == P)),            # every frame: first == ks == tau == P
    "all_tau": lambda d, P: np.all(d["tau"] == P),
    "unvoiced": lambda d, _: np.all(d["tau"] == 0),
    "voiced": lambda d, _: np.all(d["tau"] > 0),
    "some_popped": lambda d, _: np.any((d["tau"] > 0) & (d["idx"] == d["notesN"])),                  # >= 1 frame reads the popped slot
    "all_popped": lambda d, _: np.all((d["tau"] > 0) & (d["idx"] == d["notesN"])),
    "all_popped_first_tau0": lambda d, t0: np.all((d["idx"] == d["notesN"]) & (d["first"] == t0) & (d["tau"] > 0)),
    "all_idx0": lambda d, _: np.all((d["tau"] > 0) & (d["idx"] == 0)),
    "last_lag_from_below": lambda d, tm: np.any((d["first"] >= 0) & (d["first"] < tm - 1) & (d["tau"] == tm - 1)),   # the walk leaves at tauMax - 1
    "frame0_unvoiced_rest_voiced": lambda d, _: d["tau"][0] == 0 and np.all(d["tau"][1:] > 0) and len(d["tau"]) > 1,
    "any": lambda d, _: True,
}


def _case(name, fs, F, hop, length, signals, keys, expect):
    assert len(signals) == len(keys) == len(expect) == N_STREAMS and all(e[0] in PREDICATES for e in expect), name
    return EdgeCase(name, float(fs), F, hop, length, tuple(signals), tuple(keys), tuple(expect))


def _tiled_expect(P, fs):
    t0, tm = R.tau_min(fs), R.tau_max(fs)
    if P == t0 - 1:
        return ("all_at", 2 * P) if t0 <= 2 * P <= tm - 1 else ("any", None)
    return ("unvoiced", None) if P >= tm else ("all_at", P)


def _top_cases():
    out = []
    for fs, F, hop in ((44100.0, 1024, 256), (48000.0, 2048, 512)):
        t0 = R.tau_min(fs)
        for off in (0.0, 0.5, 1.0, 2.0, 3.0, 4.0):
            # (12, 0, 7): the chromatic top note 783.99 Hz lies under fs / (tau0 + 1) and no further; 739.99 Hz of keys 0 and 7 under fs / (tau0 + 4)
            chrom = ("all_popped_first_tau0", t0) if off == 0.0 else ("all_popped", None) if off <= 1.0 else ("voiced", None)
            scale = ("all_popped_first_tau0", t0) if off == 0.0 else ("all_popped", None)
            out.append(_case(f"top-fs{int(fs)}-F{F}-p{t0 + off:g}", fs, F, hop, "clamp", [("sine_p", t0 + off)] * 3, (12, 0, 7), (chrom, scale, scale)))
    return out


TILED_GEOMETRIES = ((44100.0, 1024, 256), (51200.0, 1024, 256), (8000.0, 1024, 256), (48000.0, 2048, 512), (51200.0, 2048, 512), (8000.0, 2048, 512))


def tiled_periods(fs):
    t0, tm = R.tau_min(fs), R.tau_max(fs)
    want = [t0 - 1, t0, t0 + 1, 63, 64, 65, 127, 128, 191, 192, 255, 256, 319, 320, 383, 384, 447, 448, tm - 2, tm - 1, tm]
    return sorted({P for P in want if t0 - 1 <= P <= tm})


def _tiled_cases():
    out = []
    for gi, (fs, F, hop) in enumerate(TILED_GEOMETRIES):
        Ps = tiled_periods(fs)
        Ps += Ps[:(-len(Ps)) % 3]
        for i in range(0, len(Ps), 3):
            trio = Ps[i:i + 3]
            out.append(_case(f"tiled-fs{int(fs)}-F{F}-P{'_'.join(map(str, trio))}", fs, F, hop, "clamp", [("tiled", P) for P in trio],
                             TC.KEY_SETS[(gi + i // 3) % len(TC.KEY_SETS)], [_tiled_expect(P, fs) for P in trio]))
    return out


RESIDUE_TAUMAX = (127, 128, 129, 385, 442, 443, 444, 445, 446, 447, 448, 449, 511)


def _residue_cases():
    out = []
    for i, tm in enumerate(RESIDUE_TAUMAX):
        fs = 100.0 * tm
        assert R.tau_max(fs) == tm
        for ln in ("clamp", "min"):
            out.append(_case(f"residue-tm{tm}-{ln}", fs, 1024, 256, ln, [("tiled", tm - 1), ("tc", "sine_edge"), ("tc", "saw")],
                             TC.KEY_SETS[i % len(TC.KEY_SETS)], [("all_at", tm - 1), ("last_lag_from_below", tm), ("any", None)]))
    return out


_G44 = (44100.0, 1024, 256)
UNIT_ROW = ("tc", "sine_on")


def _degenerate_cases():
    w = 1024 + R.tau_max(44100.0)
    return [
        _case("degenerate-dc", *_G44, "clamp", [("dc", 0.5), ("dc_tone", 700), ("zeros_tone", 700)], (12, 0, 7),
              [("unvoiced", None), ("frame0_unvoiced_rest_voiced", None), ("frame0_unvoiced_rest_voiced", None)]),
        _case("degenerate-impulse", *_G44, "clamp", [("impulse", 900), ("alt",), ("negzero",)], (12, 12, 12),
              [("unvoiced", None), ("all_at", 56), ("unvoiced", None)]),                       # (+-1: d is 0 at even lags; tau0 = 55 is odd)
        _case("degenerate-twins", *_G44, "clamp", [UNIT_ROW, ("scaled", 1e18, UNIT_ROW), ("scaled", 2.0 ** -60, UNIT_ROW)], (0, 0, 0),
              [("all_tau", 200), ("all_tau", 200), ("all_tau", 200)]),
    ]


BOTTOM_CASE = _case("bottom", *_G44, "clamp", [("tc", "sine_100_2")] * 3, (12, 0, 7), [("all_idx0", None)] * 3)
TOP_CASES, TILED_CASES, RESIDUE_CASES, DEGENERATE_CASES = _top_cases(), _tiled_cases(), _residue_cases(), _degenerate_cases()
CASES = TOP_CASES + [BOTTOM_CASE] + TILED_CASES + RESIDUE_CASES + DEGENERATE_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert {R.tau_max(c.fs) % 8 for c in RESIDUE_CASES} == set(range(8)) and {R.tau_max(c.fs) % 64 for c in RESIDUE_CASES} >= {63, 0, 1}


def case_id(c):
    return c.name


def length(c):
    tm = R.tau_max(c.fs)
    return c.F + tm if c.length == "min" else c.F + tm + 3 * c.hop + 17


def batch_input(c):
    """float32 [3][T]"""
    return make_rows(c.signals, length(c), c.fs, int(c.fs) + c.hop)


_REF = {}


def reference(c):
    """(period, ratio, detail) of the case from walk() and closest(), computed once (callers do not write to it); detail holds the int32
    [3][nF] tables first, ks, idx, notesN and tau (= period)."""
    if c not in _REF:
        d = {}
        p, r = R.track(batch_input(c), c.fs, c.F, c.hop, c.keys, detail=d)
        d["tau"] = p
        for a in (p, r) + tuple(d.values()):
            a.setflags(write=False)
        _REF[c] = (p, r, d)
    return _REF[c]


def holds(c, s):
    """Does stream s of the case reach the branch it is there for?"""
    name, arg = c.expect[s]
    d = {k: v[s] for k, v in reference(c)[2].items()}
    return bool(PREDICATES[name](d, arg))


# ---- the many-stream batch ----------------------------------------------------------------------------------------------------------------------
MANY_SOURCES = [c for c in CASES if (c.fs, c.F, c.hop, c.length) == (*_G44, "clamp")]


def many_rows():
    """[(case, stream)] * MANY_S: the rows of the 44100 / 1024 / 256 cases in turn, each with its own key."""
    pool = [(c, s) for c in MANY_SOURCES for s in range(N_STREAMS)]
    return [pool[i % len(pool)] for i in range(MANY_S)]


def many_input():
    """(float32 [MANY_S][T], keys [MANY_S], period [MANY_S][nF], ratio [MANY_S][nF]): every row with its three-stream result."""
    rows = many_rows()
    xs = {c: batch_input(c) for c in MANY_SOURCES}
    x = np.stack([xs[c][s] for c, s in rows])
    return x, [c.keys[s] for c, s in rows], np.stack([reference(c)[0][s] for c, s in rows]), np.stack([reference(c)[1][s] for c, s in rows])


# ---- streaming ---------------------------------------------------------------------------------------------------------------------------------
EXTRA_BLOCKS = 9            # every case runs first_decision + 9 blocks: nine decisions


def _tone_zeros_start(fs, F, N, n_blocks, run):
    """The sample from which a 196 Hz stream is silent so that exactly its last `run` blocks are unvoiced, found on the definition's raw
    periods: a start one block later shortens the run by one block."""
    W, end = SR.window_len(fs, F), n_blocks * N

    def tail(z):
        x = edge_signal(("tone_zeros", z), end, fs, 0)
        p = [int(R.track(x[None, (b + 1) * N - W:(b + 1) * N], fs, F, F)[0][0, 0]) for b in range(n_blocks - EXTRA_BLOCKS, n_blocks)]
        k = 0
        while k < len(p) and p[len(p) - 1 - k] == 0:
            k += 1
        return k, p
    lo, hi = end - W, end                                                      # the run shrinks as the silence starts later: bisect
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if tail(mid)[0] >= run:
            lo = mid
        else:
            hi = mid
    k, p = tail(lo)
    assert k == run and all(v > 0 for v in p[:len(p) - k]), (fs, F, N, run, k, p)
    return lo


_GAP = {}


def _resolve(c):
    """The case with its ("gap", run) specs replaced by the silent tail found for its geometry."""
    if c.name not in _GAP:
        sig = tuple(("tone_zeros", _tone_zeros_start(c.fs, c.F, c.N, c.n_blocks, sp[1])) if sp[0] == "gap" else sp for sp in c.signals)
        _GAP[c.name] = c._replace(signals=sig)
    return _GAP[c.name]


def _stream_case(name, fs, F, N, signals, keys, hold, glide):
    c = SC.StreamCase(name, float(fs), F, N, 0, tuple(signals), tuple(keys), hold, glide)
    return c._replace(n_blocks=SC.first_decision(c) + EXTRA_BLOCKS)


def _stream_cases():
    out = []
    follow = ((0, 1.0), (1, 0.5), (2, 0.25))
    groups = ((44100.0, 1024, 1), (44100.0, 1024, 24), (44100.0, 1024, 48), (44100.0, 1024, 63), (44100.0, 1024, 65),
              (48000.0, 2048, 100), (8000.0, 1024, 48), (51200.0, 2048, 65))
    for i, (fs, F, N) in enumerate(groups):
        hold, glide = follow[i % 3]
        tm = R.tau_max(fs)
        if N == 1:                                                                 # 1473 blocks: four streams, and no gap (a block is a sample)
            sig, keys = [("tiled", tm - 1), ("sine_p", R.tau_min(fs) + 0.5), ("tc", "sine_off"), ("tc", "saw")], (12, 0, 7, 12)
        elif (fs, N) == (44100.0, 65):                                             # 17 streams: the follow kernel's second workgroup holds one
            base = [("tiled", tm - 1), ("tiled", 64), ("sine_p", R.tau_min(fs) + 0.5), ("tc", "sine_off"), ("tc", "saw"), ("gap", hold), ("gap", hold + 1)]
            sig = [base[k % len(base)] for k in range(16)] + [("gap", hold + 1)]
            keys = tuple((12, 0, 7)[k % 3] for k in range(17))
        else:
            base = [("tiled", tm - 1), ("tiled", 64) if tm > 65 else ("tiled", tm // 2), ("sine_p", R.tau_min(fs) + 0.5), ("tc", "sine_off")]
            sig = base + ([("tc", "saw"), ("gap", 1)] if hold == 0 else [("gap", hold), ("gap", hold + 1)])    # (six streams at the most)
            keys = ((12, 0, 7, 12, 0, 7))[:len(sig)]
        out.append(_stream_case(f"edge-fs{int(fs)}-F{F}-n{N}-hold{hold}", fs, F, N, sig, keys, hold, glide))
    return out


STREAM_CASES = _stream_cases()
STREAM_BY_N = {(int(c.fs), c.F, c.N): c for c in STREAM_CASES}
assert [c.N for c in STREAM_CASES] == [1, 24, 48, 63, 65, 100, 48, 65] and sum(len(c.signals) == 17 for c in STREAM_CASES) == 1
assert all(3 <= len(c.signals) <= 6 or len(c.signals) == 17 for c in STREAM_CASES)
assert {(64 // c.N, 64 % c.N) for c in STREAM_CASES} == {(64, 0), (2, 16), (1, 16), (1, 1), (0, 64)}


def gap_streams(c):
    """[(stream, run)] of the case's streams that fall silent."""
    return [(s, sp[1]) for s, sp in enumerate(c.signals) if sp[0] == "gap"]


def stream_input(c):
    """float32 [n_blocks][S][N]: the slab the device calls take."""
    r = _resolve(c)
    x = make_rows(r.signals, c.n_blocks * c.N, c.fs, int(c.fs) + c.N)
    return np.ascontiguousarray(x.reshape(len(c.signals), c.n_blocks, c.N).transpose(1, 0, 2))


_SREF = {}


def stream_reference(c):
    """(period [n_blocks][S], followed ratio [n_blocks][S], raw ratio [n_blocks][S]) of the case in one call, computed once."""
    if c.name not in _SREF:
        t = SR.StreamTracker(len(c.signals), c.N, c.fs, c.F, c.hold, c.glide)
        p, r = t.process(stream_input(c), c.keys)
        raw = t.raw
        for a in (p, r, raw):
            a.setflags(write=False)
        _SREF[c.name] = (p, r, raw)
    return _SREF[c.name]


def stream_groupings(c):
    """SC.groupings; for N = 1 (1473 blocks) only the whole slab, the mixed pattern scaled by 97 and the pair around W."""
    if c.N > 1:
        return SC.groupings(c)
    n, fd = c.n_blocks, SC.first_decision(c)
    mixed, pat, i = [], (3 * 97, 1 * 97, 4 * 97, 2 * 97), 0
    while sum(mixed) < n:
        mixed.append(min(pat[i % len(pat)], n - sum(mixed)))
        i += 1
    return {"whole": [n], "mixed": mixed, "below-W": [fd, 1, n - fd - 1], "above-W": [fd + 1, n - fd - 1]}


# ---- the search for a long descent ----------------------------------------------------------------------------------------------------------------
def long_descent_search(n_candidates=100000, seed=5, budget_s=170.0):
    """Looks for a finite signal whose descent from `first` stops two or more ballot words behind it (see the module docstring) ->
    (candidates tried, the largest number of word boundaries a descent crossed, its description).  Not run by the suite."""
    import time
    t_end = time.time() + budget_s
    rng = np.random.default_rng(seed)
    fs, tm = 51200.0, 512
    best, tried = (-1, None), 0
    for tried in range(1, n_candidates + 1):
        if time.time() > t_end:
            break
        F = (1024, 2048)[tried % 2]
        n = F + tm
        i = np.arange(n)
        T = tm * rng.uniform(0.8, 2.0)
        chirp = rng.uniform(-0.2, 0.2) * (tried % 3 == 0)                       # relative change of the period along the row
        nh = int(rng.integers(1, 4))
        amp = np.concatenate([[1.0], rng.uniform(0.0, 0.6, nh - 1)])
        ph = np.cumsum(1.0 / (T * (1.0 + chirp * i / n)))
        x = sum(a * np.sin(2.0 * np.pi * (h + 1) * ph + rng.uniform(0, 2 * np.pi)) for h, a in enumerate(amp))
        env = ("flat", "exp_up", "exp_down", "linear", "cosine")[int(rng.integers(0, 5))]
        g = rng.uniform(0.2, 4.0)
        e = {"flat": np.ones(n), "exp_up": np.exp(g * i / n), "exp_down": np.exp(-g * i / n), "linear": 1.0 + g * i / n,
             "cosine": 1.0 + 0.9 * np.cos(2.0 * np.pi * i / (n * g))}[env]
        w = (0.5 * x * e / np.abs(x * e).max()).astype(np.float32)
        yt = R.frame_function(w, 0, fs, F, F)
        first, ks, _ = R.walk(yt, tm, fs)
        if first >= 0:
            words = min(ks, tm - 1) // 64 - first // 64
            if words > best[0]:
                best = (words, f"F {F} period {T:.1f} chirp {chirp:.2f} harmonics {np.round(amp, 2).tolist()} envelope {env} {g:.2f}: first {first} stop {ks}")
    return tried, best[0], best[1]
