"""The oracle's restatement of Notes (vpo_notes_build / vpo_notes_closest, oracle/vp_oracle.c: Notes.cpp:43-70, 79-110) against the
REFERENCE'S OWN Notes.cpp: the one translation unit of the reference that needs nothing but the standard library.  Bit for bit.

CPU only.  The reference's answers are recorded in tests/golden/ref_notes_vectors.npz (tests/golden/gen_ref_notes_vectors.py ran the
reference's Notes.cpp, compiled by oracle/Makefile `ref` / `ref-int-abs` into oracle/_ref/).  Where that compiled reference is
present as well (oracle/_ref/libnotes_ref.so), every lookup is also made on it live and must agree with the recording."""
import numpy as np
import pytest

from oracle import oracle_py as O

NOTE_RANGES = [(100.0, 800.0), (60.0, 1920.0), (27.5, 4186.0)]
N_RANDOM = 3000                         # the seeded random pitches that head every key's set (_pitches)


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(f"{golden_dir}/ref_notes_vectors.npz") as z:
        return dict(z)


def _live(key, fmin, fmax):
    """The compiled reference's Notes object, or None where oracle/_ref/libnotes_ref.so is not built."""
    return O.RefNotes(key, fmin, fmax) if O.build_ref() is not None else None


def _pitches(f, n, rng):
    # random pitches from below fMin to above fMax, every table entry (and the popped one, f[n]) with its two neighbours in double,
    # the midpoints between entries (the tie of Notes.cpp:99's `<=`), the edges
    return np.concatenate([rng.uniform(40.0, 2000.0, N_RANDOM), f[:n + 1], np.nextafter(f[:n + 1], 1e9), np.nextafter(f[:n + 1], 0.0),
                           (f[:n] + f[1:n + 1]) / 2, [0.0, 1.0, 99.9, 100.0, 800.0, 1920.0, 5000.0]])


def voiced_frame_starts(voice):
    """(stream, key, trace) of every voiced frame start of the oracle's processBlock (pitch corrector only: the side chain is not
    read) over three voice streams [3][24 * 1024] in three keys."""
    N = 1024
    for s, key in enumerate([12, 0, 7]):
        o = O.OracleStream(vocBool=0, keyPitch=key)
        o.prepare_to_play(44100.0, N)
        x = np.zeros((3, voice.shape[1]), np.float32)
        x[0] = voice[s]
        _, traces = o.run(x, trace=True)
        for fr in traces:                                    # one entry per frame start (processChunkStart)
            if not fr["gated"] and fr["pitch"] > 1:
                yield s, key, fr


def int_abs_pitches():
    return np.random.default_rng(3).uniform(100.0, 800.0, 5000)


@pytest.mark.parametrize("fmin,fmax", NOTE_RANGES)
def test_notes_restatement_equals_the_compiled_reference(golden, fmin, fmax):
    """prepare(key, fMin, fMax) (PitchProcess.cpp:98 calls it with 100 / 800) then getClosestFreq(pitch, key) for all 13 keys."""
    i = NOTE_RANGES.index((fmin, fmax))
    expect = golden[f"t1_{i}_vals"][golden[f"t1_{i}_idx"]]
    tails = np.split(golden[f"t1_{i}_tail"], np.cumsum(golden[f"t1_{i}_tail_counts"])[:-1])
    rng = np.random.default_rng(7)
    total = 0
    for key in range(13):
        ref = _live(key, fmin, fmax)
        f, n = O.notes_build(key, fmin, fmax)
        assert 0 < n <= 88
        ps = _pitches(f, n, rng)
        # the table-derived pitches are the recorded ones: the oracle's table is the one the reference's answers were taken on
        assert np.array_equal(ps[N_RANDOM:], tails[key]), f"key {key}: the oracle's note table differs from the recorded one"
        for p in ps:
            a = expect[total]
            b = O.lib().vpo_notes_closest(O._dp(f), n, float(p))
            assert a == b, f"key {key} pitch {p!r}: reference {a!r}, oracle {b!r}"
            if ref is not None:
                assert ref.closest(p, key) == a, f"key {key} pitch {p!r}: the compiled reference differs from its recording"
            total += 1
    assert total == len(expect) and total > 30000


def test_key_change_rebuilds_the_table_like_the_reference(golden):
    """getClosestFreq with a key other than the current one rebuilds the vector in place (Notes.cpp:83-88); the oracle's
    notes_get_closest does the same (vp_oracle.c).  One reference object walked through a random sequence of keys."""
    rng = np.random.default_rng(11)
    ref = _live(12, 100.0, 800.0)
    tabs = {k: O.notes_build(k, 100.0, 800.0) for k in range(13)}
    expect = golden["t2_closest"]
    assert len(expect) == 4000
    for i in range(4000):
        key = int(rng.integers(0, 13))
        p = float(rng.uniform(50.0, 1200.0))
        f, n = tabs[key]
        assert expect[i] == O.lib().vpo_notes_closest(O._dp(f), n, p)
        if ref is not None:
            assert ref.closest(p, key) == expect[i]


def test_oracle_stream_uses_the_same_lookup(golden):
    """End to end through the oracle's processBlock: at every voiced frame start the tracker's closestFreq is what the
    reference's Notes returns for the tracker's pitch (PitchProcess.cpp:593-597), in three keys."""
    seen = 0
    for s, key, fr in voiced_frame_starts(golden["t3_voice"]):
        assert seen < len(golden["t3_pitch"]), "more voiced frame starts than recorded"
        assert (s, fr["pitch"]) == (golden["t3_stream"][seen], golden["t3_pitch"][seen]), "the tracker's pitch differs from the recorded one"
        assert fr["closestFreq"] == golden["t3_closest"][seen]
        ref = _live(key, 100.0, 800.0)
        if ref is not None:
            assert ref.closest(fr["pitch"], key) == golden["t3_closest"][seen]
        assert fr["beta"] == fr["closestFreq"] / fr["pitch"]
        seen += 1
    assert seen == len(golden["t3_pitch"]) and seen > 20


def test_the_int_abs_reading_of_notes_cpp_99_differs(golden):
    """SURVEY.md Q1, for the record: compiled WITHOUT `-include math.h`, this image's libstdc++ resolves Notes.cpp:99's unqualified
    abs() to int abs(int) and the reference picks the farther note whenever the two distances share their integer part.  The oracle
    (and the HIP path) follow the floating overload -- the author's platform's.  Both readings' answers are recorded
    (oracle/Makefile `ref-int-abs` built the other one)."""
    ps = int_abs_pitches()
    int_abs, good = golden["t4_int_abs"], golden["t4_closest"]
    assert len(int_abs) == len(good) == len(ps)
    f, n = O.notes_build(12, 100.0, 800.0)
    ref = _live(12, 100.0, 800.0)
    for i, p in enumerate(ps):
        assert good[i] == O.lib().vpo_notes_closest(O._dp(f), n, float(p))
        if ref is not None:
            assert ref.closest(float(p), 12) == good[i]
    diff = int((int_abs != good).sum())
    assert 0 < diff < 0.05 * len(ps), diff
