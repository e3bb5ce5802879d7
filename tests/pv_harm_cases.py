"""The harmonizer's test matrix (vp_stft_harmonize, vp_hz_process_blocks_device): voice sets, gains, dry values and the cases on which
the definition's mutants must show, shared by tests/test_pv_harm_reference_cpu.py and tests/test_gpu_pv_harm.py.  Test infrastructure
only.  The definition is tests/pv_harm_reference.py.

Inputs and per-voice references are the peak-locked matrix's: a voice set uses only curves of pv_lock_cases.GPU_CURVES on
pv_lock_cases.gpu_input, so every voice's reference is pv_lock_cases.gpu_reference -- cached, and what the locked GPU tests already hold
the locked kernel to.  The bound of every pointwise comparison is pv_harm_reference.gpu_bound's."""
import numpy as np

import pv_harm_reference as HR
import pv_lock_cases as LC
from stft_reference import stft_roundtrip

F = LC.F
S = len(LC.GPU_STREAMS)
HOPS = LC.GPU_HOPS
NFS = LC.GPU_NF
TEETH = LC.TEETH

# V -> the curves of its voices
VOICE_SETS = {1: ("steps",), 2: ("+7", "-12"), 3: ("+7", "vibrato", "steps"), 4: ("-12", "octaves", "outside", "vibrato")}
for _c in VOICE_SETS.values():
    assert set(_c) <= set(LC.GPU_CURVES)

# per-stream gains [S][4] (a voice set of V voices takes the first V columns: every set sees a 0, a negative, a 4.0 and a NaN) and dry [S]
_NAN = float("nan")
GAINS = np.array([[1.0, 0.5, 0.25, 0.75],
                  [0.0, 1.0, -0.5, 0.3],
                  [-1.0, 0.7, 4.0, 0.2],
                  [4.0, _NAN, 1.0, -0.25],
                  [0.5, 0.5, 0.0, _NAN],
                  [_NAN, -2.0, 1.0, 1.0]])
DRY = np.array([0.0, 1.0, 0.5, 1.0, 0.0, 0.5])
assert GAINS.shape == (S, HR.MAX_VOICES) and DRY.shape == (S,)


def gains(V):
    return np.ascontiguousarray(GAINS[:, :V])


def ratios(V, hop, nF):
    """[S][V][nF] float64 ratios (unclamped), every stream its own phase of each curve."""
    return np.ascontiguousarray(np.stack([LC.gpu_ratios(c, hop, nF) for c in VOICE_SETS[V]], axis=1))


_RT = {}


def roundtrip(hop, nF):
    """stft_roundtrip of pv_lock_cases.gpu_input, float64 [S][T], once per case (callers do not write to it)."""
    if (hop, nF) not in _RT:
        x = LC.gpu_input(hop, nF)
        y = np.stack([stft_roundtrip(x[s], F, hop) for s in range(S)])
        y.setflags(write=False)
        _RT[(hop, nF)] = y
    return _RT[(hop, nF)]


def voice_refs(V, hop, nF):
    """The voices' locked references, [V] arrays [S][T]."""
    return [LC.gpu_reference(hop, nF, c) for c in VOICE_SETS[V]]


def reference(V, hop, nF, gain="case", dry="case"):
    """(ref float64 [S][T], bound [S]) of one GPU case from the cached parts; gain / dry: "case" (the tables above), None, or a table."""
    g = gains(V) if isinstance(gain, str) else gain
    d = DRY if isinstance(dry, str) else dry
    rt, refs = roundtrip(hop, nF), voice_refs(V, hop, nF)
    ref, bnd = [], []
    for s in range(S):
        gs, ds = None if g is None else g[s], None if d is None else d[s]
        ref.append(HR.from_parts(rt[s], [r[s] for r in refs], gs, ds))
        bnd.append(HR.gpu_bound(hop, ds, rt[s], gs, [r[s] for r in refs]))
    return np.stack(ref), np.array(bnd)


# ---- teeth: mutant -> (V, hop, nF) of the GPU case chosen to see it (streams "voice" and "glide" carry partials whose angles matter) ---
TEETH_CASES = {
    "shared_theta": (3, 256, 8),
    "swapped": (2, 256, 8),
    "nodry": (3, 256, 8),
    "gain_first_voice": (3, 256, 8),
}
assert set(TEETH_CASES) == set(HR.MUTANTS)


# ---- streaming ----------------------------------------------------------------------------------------------------------------------------
STREAM_V = 3
STREAM_DRY = 0.5
STREAM_BLOCKS = LC.STREAM_BLOCKS
STREAM_CALLS = LC.STREAM_CALLS


def stream_ratios(hop, N):
    """[n_blocks][S][V] ratios, some outside the clamp."""
    nb = LC.stream_blocks(N)
    return LC.ratio_of(np.random.default_rng([hop, N, 51]).uniform(-13.0, 13.0, (nb, S, STREAM_V)))


def per_frame(table, N, hop, T):
    """[n_blocks][S][V] -> the one-shot's [S][V][nFrames]: a frame takes the block in which its last sample arrives."""
    nF = (T - F) // hop + 1
    blk = (np.arange(nF) * hop + F - 1) // N
    return np.ascontiguousarray(np.asarray(table)[blk].transpose(1, 2, 0))
