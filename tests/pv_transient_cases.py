"""The transient-preserving stretch's test matrix (vp_stft_onset_flux, vp_onset_pick, vp_stretch_positions_transient,
vp_stft_time_stretch_locked_reset): the signals, cases and items that tests/test_pv_transient_reference_cpu.py (gate, probe, teeth, plan,
pick, margins, quality), tests/test_gpu_pv_onset.py and tests/test_gpu_pv_transient.py (kernels against NumPy) and
tools/pv_transient_quality.py iterate.  Test infrastructure only.  The definition is tests/pv_transient_reference.py; the stage's bound,
gate tolerance, teeth and conditioning probe are tests/pv_stretch_lock_cases.py's, unchanged -- a reset removes accumulated angle and adds
no sensitivity.

  flux cases     rows [S][n_in] for the flux kernel: nG = 1, 2, NWV, NWV + 1; one frame either side of a chunk boundary (chunks hold
                 CHUNK = 15 frames when the batch is small); n_in = F and F + 1 (odd: odd rows unaligned); every hop; a silent and a NaN row
                 beside good rows; 300 short rows.  The bound per frame is pv_transient_reference.flux_bound's (derived, not measured).
  pick cases     the rows whose FLAGS the GPU test compares: bursts and plucks on a low noise floor, every hop.  Every comparison of every
                 frame keeps PICK_MARGIN = 1e-6 mass from its edge in the definition (asserted on the CPU), except `flux[0] > 0`, whose
                 left side is the constant 0 on both sides.  Steady noise sits close to the threshold at hop 512 and is kept out.
  stage items    pv_stretch_lock_cases.gpu_items with a reset table per stream (frame 0, the last frame, every frame, scattered frames,
                 garbage bytes), and the silent items: a flag on a silent frame and on the frame behind a silent one.
  teeth          mutant -> the case that sees it (TEETH_CASES).
  quality        bursts and plucks, stretch 0.5, 0.75, 1.5, 2, hops 128, 256, 512, with and without +7 semitones.
"""
from collections import namedtuple

import numpy as np

import pv_lock_cases as LC
import pv_stretch_lock_cases as K
import pv_stretch_lock_reference as SLR
import pv_transient_reference as TR

F = LC.F
FS = LC.FS
NWV = 4                                     # csrc/vp_stft.h VP_STFT_WAVES
CHUNK = 4 * NWV - 1                         # csrc/vp_stft_onset.inc VP_ONSET_CHUNK_MIN: a small batch's frames per chunk
HOPS = K.HOPS
THR = 0.2                                   # include/vp_amd.h VP_DEFAULT_ONSET_THRESHOLD
PICK_MARGIN = 1e-6
GATE_TOL, TEETH, bound = K.GATE_TOL, K.TEETH, K.bound
CONDITION_EPS, CONDITION_SEEDS, CONDITION_SHARE = K.CONDITION_EPS, K.CONDITION_SEEDS, K.CONDITION_SHARE


# ---- signals (float32, seeded) --------------------------------------------------------------------------------------------------------------
def bursts(n, onsets, seed=0, floor=0.0, tau=1500.0):
    """Decaying noise bursts from the samples `onsets` on; digital silence in front of the first unless floor > 0 (a steady noise floor)."""
    rng = np.random.default_rng([seed, 71])
    t = np.arange(n)
    x = floor * rng.standard_normal(n)
    for t0 in onsets:
        x += np.where(t >= t0, 0.25 * np.exp(-np.maximum(t - t0, 0) / tau), 0.0) * rng.standard_normal(n)
    return x.astype(np.float32)


def plucks(n, onsets, seed=0, floor=0.0, tau=4000.0):
    """Plucked harmonic notes: eight harmonics, the higher ones decaying faster, a new note at every onset."""
    rng = np.random.default_rng([seed, 72])
    t = np.arange(n)
    x = floor * rng.standard_normal(n)
    for i, t0 in enumerate(onsets):
        f0 = (196.0, 261.6, 329.6, 392.0)[i % 4]
        for h in range(1, 9):
            x += np.where(t >= t0, 0.3 / h * np.exp(-np.maximum(t - t0, 0) * h / tau) * np.sin(2 * np.pi * f0 * h * (t - t0) / FS), 0.0)
    return x.astype(np.float32)


ATTACKS = {"bursts": bursts, "plucks": plucks}


def in_length(nG, hop, extra=0):
    return F + (nG - 1) * hop + extra


# ---- the flux cases ---------------------------------------------------------------------------------------------------------------------------
FluxCase = namedtuple("FluxCase", "name hop n_in rows")
_MIX = ("noise", "voice", "bursts", "tone-tone", "plucks")


def _flux_cases():
    cs = []
    for nG in (1, 2, NWV, NWV + 1):
        cs.append(FluxCase(f"nG{nG}", 256, in_length(nG, 256, 255 if nG == 2 else 0), _MIX[:3]))
    for nG in (CHUNK, CHUNK + 1, CHUNK + 2, 2 * CHUNK, 2 * CHUNK + 1):                   # the last frame of a chunk, the first and second of the next
        cs.append(FluxCase(f"chunk-nG{nG}", 64, in_length(nG, 64, 1), _MIX))
    cs.append(FluxCase("n_in-F", 256, F, _MIX[:3]))
    cs.append(FluxCase("n_in-F+1", 256, F + 1, _MIX[:4]))
    for hop in HOPS:
        cs.append(FluxCase(f"hop{hop}", hop, in_length(21, hop, hop - 1) | 1, _MIX))
    return cs


FLUX_CASES = _flux_cases()


def row(name, n, seed, hop=256, floor=0.0):
    if name in ATTACKS:
        first = min(F + 2 * hop + 37, max(n - F, 1))
        onsets = [t0 for t0 in (first, first + (n - first) // 2 + 11) if t0 < n]
        return ATTACKS[name](n, onsets, seed, floor)
    return LC.SIGNALS[name](n, seed=seed)


def flux_input(c):
    return np.stack([row(r, c.n_in, c.hop + i, c.hop) for i, r in enumerate(c.rows)])


BIG_S, BIG_HOP, BIG_N_IN = 300, 256, in_length(5, 256, 3)


def big_flux_input():
    x = (0.25 * np.random.default_rng([BIG_S, 73]).standard_normal((BIG_S, BIG_N_IN))).astype(np.float32)
    x *= (1.0 + np.arange(BIG_S, dtype=np.float32))[:, None] / BIG_S                     # (every row its own level: a row written by another's workgroup shows)
    return x


_FLUX = {}


def flux_reference(x, hop, key):
    """(flux, mass, bound) float64 [S][nG], once per key (callers do not write to it)."""
    if key not in _FLUX:
        fm = [TR.onset_flux(r, F, hop) for r in x]
        out = (np.stack([a for a, _ in fm]), np.stack([b for _, b in fm]), np.stack([TR.flux_bound(r, F, hop) for r in x]))
        for a in out:
            a.setflags(write=False)
        _FLUX[key] = out
    return _FLUX[key]


# ---- the pick cases: rows whose flags the GPU must reproduce ----------------------------------------------------------------------------------
PickCase = namedtuple("PickCase", "name hop n_in")
PICK_FLOOR = 1e-3
PICK_CASES = [PickCase(f"pick-hop{hop}", hop, in_length(40, hop, 5) | 1) for hop in HOPS]
PICK_ROWS = ("bursts", "plucks", "bursts", "plucks")


def pick_input(c):
    return np.stack([row(r, c.n_in, 7 * c.hop + i, c.hop, PICK_FLOOR) for i, r in enumerate(PICK_ROWS)])


def margins_ok(flux, mass, thr=THR):
    """Whether every comparison of every frame keeps PICK_MARGIN mass from its edge; `flux[0] > 0` is exempt (a constant on both sides).
    Returns (ok, the smallest margin)."""
    m = TR.pick_margins(flux, mass, thr)
    m[0, 0] = np.inf
    return bool(m.min() >= PICK_MARGIN), float(m.min())


# ---- the stage items: the locked stretch's GPU items with a reset table -----------------------------------------------------------------------
Item = namedtuple("Item", "name hop x pos T ratio reset")
GPU_CASES, gpu_id, N_STREAMS = K.GPU_CASES, K.gpu_id, K.N_STREAMS


def reset_rows(nF, key):
    """uint8 [N_STREAMS][nF]: frame 0; the last frame; every frame; scattered frames; garbage bytes (any non-zero byte is a set flag)."""
    r = np.zeros((N_STREAMS, nF), np.uint8)
    r[0, 0] = 1
    r[1, nF - 1] = 1
    r[2, :] = 1
    r[3, [f for f in (3, 4, 11) if f < nF]] = 1
    g = np.random.default_rng([key, 74]).integers(0, 4, nF)
    r[4] = np.where(g == 0, np.random.default_rng([key, 75]).integers(1, 256, nF), 0)
    r[4, nF // 2] = 0x80
    return r


def gpu_items(c):
    rs = reset_rows(c.nF, c.hop + c.nF)
    return [Item(it.name + "-reset", it.hop, it.x, it.pos, it.T, it.ratio, rs[s]) for s, it in enumerate(K.gpu_items(c))]


SILENT_HOP, SILENT_NF = 256, 19
SILENT_FRAMES = tuple(range(8, 15))         # frames that lie inside the zeroed samples at positions f hop; frame 15 is the frame behind


def silent_items():
    """Noise with samples [2048, 4608) zeroed, read at f hop: frames 8 .. 14 have no peak.  Streams: a flag on a silent frame and on the
    frame behind the silent ones; flags on all of those; the same at +7 semitones; a flag on the last silent frame only."""
    hop, nF = SILENT_HOP, SILENT_NF
    T = LC.length(nF, hop, 3)
    pos = np.arange(nF, dtype=np.int64) * hop
    items = []
    for s, (frames, semis) in enumerate((((9, 15), 0.0), (tuple(range(8, 16)), -5.0), ((9, 15), 7.0), ((14,), 7.0))):
        x = LC.noise(T + 1, seed=80 + s).copy()
        x[2048:4608] = 0.0
        reset = np.zeros(nF, np.uint8)
        reset[list(frames)] = 1
        items.append(Item(f"silent-s{s}", hop, x, pos, T, np.full(nF, K.ratio_of(semis)), reset))
    return items


_REF = {}


def reference(it, form="a", mutant=None):
    """float64 [T], once per item, form and mutant (callers do not write to it)."""
    key = (it.name, form, mutant)
    if key not in _REF:
        if form == "b":
            y = TR.stretch_locked_reset_roundtrip_b(it.x, it.pos, it.T, it.ratio, it.reset, F, it.hop)
        else:
            y = TR.stretch_locked_reset_roundtrip(it.x, it.pos, it.T, it.ratio, it.reset, F, it.hop, mutant)
        y.setflags(write=False)
        _REF[key] = y
    return _REF[key]


def gate_and_probe(it):
    """pv_stretch_lock_cases.gate_and_probe with the reset table."""
    y = reference(it)
    gate = np.abs(y - reference(it, "b")).max() / max(1.0, float(np.abs(y).max()))
    moved = max(np.abs(TR.stretch_locked_reset_roundtrip(it.x, it.pos, it.T, it.ratio, it.reset, F, it.hop, perturb=(CONDITION_EPS, s)) - y).max()
                for s in CONDITION_SEEDS)
    return gate, moved / bound(it.hop, y)


# items that miss the conditioning probe: properties only (finite and bounded), by name
DEMOTED = ()


def pointwise(it):
    return it.name not in DEMOTED


ceiling = K.ceiling


# ---- the identity after a reset ----------------------------------------------------------------------------------------------------------------
IDENTITY_R = 7                              # frames 0 .. 6 at +7 semitones and a stretch of 0.8, frame 7 flagged, ratio 1 and hop apart from there
IDENTITY_NF = 19


def identity_tables(hop, n_streams):
    """(pos int64 [S][nF], ratio [S][nF], reset uint8 [S][nF], n_in): ratio != 1 and D != hop up to frame r, then the reset."""
    nF, r = IDENTITY_NF, IDENTITY_R
    pos = np.zeros((n_streams, nF), np.int64)
    for s in range(n_streams):
        head = K.factor_positions(r + 1, hop, (0.8, 1.37, 0.5, 1.0)[s % 4])
        pos[s, :r + 1] = head
        pos[s, r:] = head[r] + np.arange(nF - r) * hop
    ratio = np.ones((n_streams, nF))
    ratio[:, :r] = K.ratio_of(7.0)
    reset = np.zeros((n_streams, nF), np.uint8)
    reset[:, r] = 1
    return pos, ratio, reset, F + int(pos.max()) + 2


# ---- teeth: mutant -> the case that sees it ------------------------------------------------------------------------------------------------------
TEETH_CASES = {
    "noreset": ("stage", K.GpuCase(256, 19, "+7"), 3),          # a voice at +7 with flags on frames 3, 4 and 11: the angles must restart there
    "late_reset": ("stage", K.GpuCase(256, 19, "+7"), 3),
    "reset_prev": ("stage", K.GpuCase(256, 19, "vibrato"), 3),  # ratio != 1 behind the flag: the next unwrap needs the flagged frame's phases
    "norect": ("flux", "bursts", 256),                          # decaying bursts: most of the difference is negative
    "flux_next": ("flux", "bursts", 256),
    "pick_ge": ("pick", np.array([0.0, 1.0, 1.0, 0.5, 0.0]), np.array([2.0, 2.0, 2.0, 2.0, 2.0])),      # a plateau: its left end only
    "fc_floor": ("plan", dict(nF=60, hop=256, stretch=1.5, n_in=F + 45 * 256, K=2, onsets=(15,))),     # g stretch = 22.5: rounds to 23, floors to 22
    "span_short": ("plan", dict(nF=60, hop=256, stretch=1.5, n_in=F + 45 * 256, K=2, onsets=(16,))),
}


def teeth_stage_item(mutant):
    _, c, s = TEETH_CASES[mutant]
    return gpu_items(c)[s]


def plan_of(spec, mutant=None, why=None):
    nG = (spec["n_in"] - F) // spec["hop"] + 1
    on = np.zeros(nG, np.uint8)
    on[list(spec["onsets"])] = 1
    return TR.plan_positions(on, spec["nF"], spec["hop"], spec["stretch"], spec["n_in"], F, spec["K"], mutant, why)


# ---- quality: what the scheme is for ------------------------------------------------------------------------------------------------------------
QUALITY_STRETCHES = (0.5, 0.75, 1.5, 2.0)
QUALITY_HOPS = (128, 256, 512)
QUALITY_WINDOW = 600                        # samples around an onset compared with the input's
PRE_SAMPLES, POST_SAMPLES = int(0.030 * FS), int(0.014 * FS)
QualityCase = namedtuple("QualityCase", "signal stretch hop")
QUALITY_CASES = [QualityCase(s, a, hop) for s in ATTACKS for a in QUALITY_STRETCHES for hop in QUALITY_HOPS]


def quality_id(c):
    return f"{c.signal}-x{c.stretch:g}-hop{c.hop}"


def quality_input(c, n_onsets=3):
    """(x float32, the true onsets in samples): onsets 11 000 samples apart, deliberately off the frame grid."""
    onsets = [9011 + 10987 * i for i in range(n_onsets)]
    n = onsets[-1] + 9000
    return ATTACKS[c.signal](n, onsets, seed=c.hop), onsets


def _rms(a):
    return float(np.sqrt(np.mean(np.square(a)))) if len(a) else 0.0


def onset_distance(y, x, t_out, t_in, search=0):
    """The relative rms distance of the QUALITY_WINDOW output samples around t_out from the input's around t_in; with `search`, the
    smallest over output lags of up to that many samples either way (the baseline has no exact landing point: it gets the best)."""
    h = QUALITY_WINDOW // 2
    ref = np.asarray(x, np.float64)[t_in - h:t_in + h]
    best = np.inf
    for lag in range(-search, search + 1):
        a = t_out + lag - h
        if a < 0 or a + 2 * h > len(y):
            continue
        best = min(best, _rms(y[a:a + 2 * h] - ref) / _rms(ref))
    return best


def pre_post(y, t_out):
    """rms of the 30 ms before the onset over rms of the 14 ms after it."""
    return _rms(y[max(t_out - PRE_SAMPLES, 0):t_out]) / max(_rms(y[t_out:t_out + POST_SAMPLES]), 1e-300)


def quality(c, semitones=0.0, n_onsets=3, thr=THR):
    """One case measured on the definitions: a dict with the onsets found and true, and per true onset the distance and the pre/post ratio
    with the scheme (`new`) and with the locked stretch as it is (`old`)."""
    x, onsets = quality_input(c, n_onsets)
    hop, a = c.hop, c.stretch
    n_in = len(x)
    T = int(n_in * a)
    nF = (T - F) // hop + 1
    r = K.ratio_of(semitones)
    y_new, pos, reset, on = TR.transient_stretch(x, a, thr, F, hop, None, r, T)
    base = np.minimum(np.floor(np.arange(nF) * hop / a), n_in - F).astype(np.int64)
    y_old = SLR.stretch_locked_roundtrip(x, base, T, r, F, hop)
    Kspan = TR.default_span(F, hop)
    found = [int(g) for g in np.nonzero(on)[0]]
    true = [(t0 - F // 2) / hop for t0 in onsets]
    rows = []
    for t0 in onsets:
        g = min(found, key=lambda v: abs(v - (t0 - F // 2) / hop)) if found else None
        fc = int(np.floor(g * a + 0.5)) if g is not None else None
        accepted = g is not None and fc - Kspan >= 0 and fc - Kspan < nF and reset[fc - Kspan] != 0
        t_new = t0 + (fc - g) * hop if accepted else int(round((t0 - F // 2) * a + F // 2))
        t_old = int(round((t0 - F // 2) * a + F // 2))
        rows.append(dict(onset=t0, frame=g, accepted=bool(accepted),
                         new=onset_distance(y_new, x, t_new, t0), old=onset_distance(y_old, x, t_old, t0, search=hop),
                         new_pre=pre_post(y_new, t_new), old_pre=pre_post(y_old, t_old)))
    return dict(found=found, true=true, rows=rows)
