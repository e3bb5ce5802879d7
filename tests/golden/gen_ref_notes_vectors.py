"""Generate tests/golden/ref_notes_vectors.npz: what the REFERENCE's own Notes.cpp returns (oracle/_ref/libnotes_ref.so, and its
int-abs reading oracle/_ref/libnotes_ref_int_abs.so; oracle/Makefile `ref`, `ref-int-abs`) for every lookup that
tests/test_oracle_ref_notes.py makes, so that the test runs where the reference tree is not.

Only inputs and outputs (data) are stored -- no reference source.  The reference tree exists only in the build container, so this
script is run once there and its output committed.

    python tests/golden/gen_ref_notes_vectors.py

Stored per test (the pitches that come from a seeded generator alone are drawn again by the test, in the same order):
  t1_{i}_*  parametrisation i of test_notes_restatement_equals_the_compiled_reference: the table-derived pitches of every key
            (`tail`, `tail_counts`), and the reference's closest note of every pitch in the test's order, as an index (`idx`) into the
            sorted distinct answers (`vals`)
  t2_closest  test_key_change_rebuilds_the_table_like_the_reference: the 4000 answers of one reference object
  t3_*      test_oracle_stream_uses_the_same_lookup: the three synthetic voice streams it runs (vocoderproject_amd.synth, float32),
            and per voiced frame start the tracker's pitch and the reference's closest note
  t4_*      test_the_int_abs_reading_of_notes_cpp_99_differs: both readings' answers for the 5000 pitches
"""
import ctypes as C
import os
import subprocess
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

from oracle import oracle_py as O  # noqa: E402
import test_oracle_ref_notes as T  # noqa: E402  (the test's own pitch sets and parameters)


def main():
    assert O.build_ref() is not None, "oracle/_ref/libnotes_ref.so cannot be built here (no reference tree)"
    out = {}
    for i, (fmin, fmax) in enumerate(T.NOTE_RANGES):
        rng = np.random.default_rng(7)
        tails, counts, closest = [], [], []
        for key in range(13):
            ref = O.RefNotes(key, fmin, fmax)
            f, n = O.notes_build(key, fmin, fmax)
            ps = T._pitches(f, n, rng)
            tail = ps[T.N_RANDOM:]
            tails.append(tail)
            counts.append(len(tail))
            closest += [ref.closest(p, key) for p in ps]
        vals, idx = np.unique(np.array(closest), return_inverse=True)
        assert len(vals) < 1 << 16
        out[f"t1_{i}_tail"] = np.concatenate(tails)
        out[f"t1_{i}_tail_counts"] = np.array(counts, np.int32)
        out[f"t1_{i}_vals"] = vals
        out[f"t1_{i}_idx"] = idx.astype(np.uint16)

    rng = np.random.default_rng(11)
    ref = O.RefNotes(12, 100.0, 800.0)
    t2 = []
    for _ in range(4000):
        key = int(rng.integers(0, 13))
        p = float(rng.uniform(50.0, 1200.0))
        t2.append(ref.closest(p, key))
    out["t2_closest"] = np.array(t2)

    from vocoderproject_amd.synth import make_streams
    voice = np.ascontiguousarray(make_streams(3, 1024 * 24).numpy()[:, 0])
    pitch, closest, stream = [], [], []
    for s, key, fr in T.voiced_frame_starts(voice):
        ref = O.RefNotes(key, 100.0, 800.0)
        pitch.append(fr["pitch"])
        closest.append(ref.closest(fr["pitch"], key))
        stream.append(s)
    out["t3_voice"] = voice
    out["t3_stream"] = np.array(stream, np.int32)
    out["t3_pitch"] = np.array(pitch)
    out["t3_closest"] = np.array(closest)

    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref-int-abs"])
    R = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libnotes_ref_int_abs.so"))
    R.refnotes_new.restype = C.c_void_p
    R.refnotes_prepare.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
    R.refnotes_closest.argtypes = [C.c_void_p, C.c_double, C.c_int]
    R.refnotes_closest.restype = C.c_double
    h = R.refnotes_new()
    R.refnotes_prepare(h, 12, 100.0, 800.0)
    good = O.RefNotes(12, 100.0, 800.0)
    ps = T.int_abs_pitches()
    out["t4_int_abs"] = np.array([R.refnotes_closest(h, float(p), 12) for p in ps])
    out["t4_closest"] = np.array([good.closest(float(p), 12) for p in ps])

    path = os.path.join(HERE, "ref_notes_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
