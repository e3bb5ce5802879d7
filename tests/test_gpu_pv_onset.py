"""The onset flux on the GPU (include/vp_amd.h vp_stft_onset_flux; kernel vp_k_stft_onset_flux of csrc/vp_stft_onset.inc) against the NumPy
definition tests/pv_transient_reference.py on the rows of tests/pv_transient_cases.py: nG = 1, 2, NWV, NWV + 1, one frame either side of a
chunk boundary, n_in = F and F + 1, every hop, a silent and a NaN row beside good rows, more rows than compute units; the flags picked
from the GPU's tables; argument errors; no allocation.  The tables start as NaN, so every entry must have been written.

The asserted bound is DERIVED, per frame: both sides are double-precision transforms of the same float32 samples, so the difference is
rounding, at most 4 * 513 * log2(F) * 2^-53 * (||x_g w||_2 + ||x_(g-1) w||_2) (pv_transient_reference.flux_bound; 4 is margin over the
usual FFT error constant).  A wrong predecessor, a missing bin or a missing rectifier is off by orders of magnitude more
(tests/test_pv_transient_reference_cpu.py: the flux mutants are 1e6 bounds away).  The ONSET lines (-s) are the measured errors."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pv_transient_cases as TC  # noqa: E402
import pv_transient_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu

F = TC.F
VP_ERR_INVALID_ARG, VP_ERR_GEOMETRY = -1, -4


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _flux(x, hop):
    """One vp_stft_onset_flux call on x [S][n_in] -> (flux, mass) float64 [S][nG], from tables prefilled with NaN."""
    from vocoderproject_amd import StftRoundTrip
    S, n_in = x.shape
    nG = (n_in - F) // hop + 1
    st = StftRoundTrip(S, F + hop, F, hop)                                               # (the handle's own length plays no part)
    d_flux = torch.full((S, nG), float("nan"), dtype=torch.float64, device="cuda")
    d_mass = torch.full((S, nG), float("nan"), dtype=torch.float64, device="cuda")
    st.onset_flux(_dev(x, np.float32), d_flux, d_mass)
    torch.cuda.synchronize()
    st.close()
    return d_flux.cpu().numpy(), d_mass.cpu().numpy()


def _check(flux, mass, x, hop, key, tag):
    want_flux, want_mass, bnd = TC.flux_reference(x, hop, key)
    assert flux.shape == want_flux.shape and np.all(np.isfinite(flux)) and np.all(np.isfinite(mass)), tag
    assert np.all(flux[:, 0] == 0)
    worst = 0.0
    for s in range(len(x)):
        ef, em = np.abs(flux[s] - want_flux[s]), np.abs(mass[s] - want_mass[s])
        share = max(float((ef / bnd[s].clip(1e-300)).max()), float((em / bnd[s].clip(1e-300)).max()))
        worst = max(worst, share)
        assert np.all(ef <= bnd[s]) and np.all(em <= bnd[s]), (tag, s, float(ef.max()), float(em.max()), float(bnd[s].min()))
    print(f"ONSET {tag}: S {len(x)} nG {flux.shape[1]} hop {hop}: largest error {worst:.3g} of the derived bound")


@pytest.mark.parametrize("c", TC.FLUX_CASES, ids=lambda c: c.name)
def test_flux_and_mass_match_numpy(c):
    x = TC.flux_input(c)
    assert x.shape == (len(c.rows), c.n_in)
    flux, mass = _flux(x, c.hop)
    _check(flux, mass, x, c.hop, c.name, c.name)


def test_the_shapes_the_cases_claim():
    nG = {c.name: (c.n_in - F) // c.hop + 1 for c in TC.FLUX_CASES}
    assert [nG[f"nG{n}"] for n in (1, 2, TC.NWV, TC.NWV + 1)] == [1, 2, TC.NWV, TC.NWV + 1]
    assert [nG[f"chunk-nG{n}"] for n in (15, 16, 17, 30, 31)] == [15, 16, 17, 30, 31] and TC.CHUNK == 15
    assert nG["n_in-F"] == 1 and nG["n_in-F+1"] == 1
    assert all(c.n_in % 2 == 1 for c in TC.FLUX_CASES if c.name.startswith(("hop", "chunk")))   # odd rows: every second row unaligned
    from vocoderproject_amd import load_library
    chunk = getattr(load_library(), "_Z19vp_stft_onset_chunkii")                          # int vp_stft_onset_chunk(int nG, int nStreams)
    assert chunk(17, 5) == TC.CHUNK and chunk(31, 5) == TC.CHUNK and chunk(253, 256) == 127 and chunk(5, 300) == TC.CHUNK


def test_a_silent_and_a_nan_row_touch_no_other_row():
    """Rows are independent: beside a silent row and a row of NaN the good rows have the bits they have alone (another S: another
    partition into chunks), the silent row is exactly 0 and the NaN row stays NaN."""
    hop = 128
    c = TC.FluxCase("beside", hop, TC.in_length(37, hop, 1), ("bursts", "voice", "plucks"))
    good = TC.flux_input(c)
    x = np.stack([good[0], np.zeros(c.n_in, np.float32), good[1], np.full(c.n_in, np.nan, np.float32), good[2]])
    flux, mass = _flux(x, hop)
    assert np.all(flux[1] == 0) and np.all(mass[1] == 0)
    assert np.all(np.isnan(mass[3])) and np.all(np.isnan(flux[3, 1:])) and flux[3, 0] == 0
    _check(flux[[0, 2, 4]], mass[[0, 2, 4]], good, hop, "beside", "beside a silent and a NaN row")
    for s, row in zip((0, 2, 4), good):
        f1, m1 = _flux(row[None], hop)
        assert np.array_equal(f1[0], flux[s]) and np.array_equal(m1[0], mass[s]), s


def test_more_rows_than_compute_units():
    """300 short rows, every one its own noise at its own level: each is compared, so a row written by another's workgroup shows."""
    x = TC.big_flux_input()
    flux, mass = _flux(x, TC.BIG_HOP)
    _check(flux, mass, x, TC.BIG_HOP, "big", "300 rows")
    assert len(x) == TC.BIG_S > 256 and mass.min() > 0


@pytest.mark.parametrize("c", TC.PICK_CASES, ids=lambda c: c.name)
def test_flags_picked_from_the_gpu_tables_equal_the_definitions(c):
    from vocoderproject_amd import pick_onsets
    x = TC.pick_input(c)
    flux, mass = _flux(x, c.hop)
    want_flux, want_mass, _ = TC.flux_reference(x, c.hop, c.name)
    _check(flux, mass, x, c.hop, c.name, c.name)
    for s in range(len(x)):
        got, want = pick_onsets(flux[s], mass[s], TC.THR), TR.pick_onsets(want_flux[s], want_mass[s], TC.THR)
        assert want.any() and np.array_equal(got, want), (c.name, s, np.nonzero(got)[0], np.nonzero(want)[0])


def test_bad_arguments_are_refused_and_write_nothing_and_calls_allocate_nothing():
    from vocoderproject_amd import StftRoundTrip, VpError
    hop, S = 256, 3
    x = TC.flux_input(TC.FluxCase("args", hop, TC.in_length(9, hop), ("noise", "voice", "bursts")))
    n_in = x.shape[1]
    nG = (n_in - F) // hop + 1
    st = StftRoundTrip(S, F + hop, F, hop)
    d_in = _dev(x, np.float32)
    d_flux = torch.full((S, nG), float("nan"), dtype=torch.float64, device="cuda")
    d_mass = torch.full((S, nG), float("nan"), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    call = st.L.vp_stft_onset_flux
    good = dict(p=st.h, d_in=d_in.data_ptr(), n_in=n_in, d_flux=d_flux.data_ptr(), d_mass=d_mass.data_ptr())
    for change in (dict(n_in=F - 1), dict(n_in=0), dict(d_in=None), dict(d_flux=None), dict(d_mass=None)):
        a = dict(good, **change)
        assert call(a["p"], a["d_in"], a["n_in"], a["d_flux"], a["d_mass"], stream) == VP_ERR_INVALID_ARG, change
        assert b"onset flux" in st.L.vp_stft_last_error(st.h)
    assert call(None, good["d_in"], n_in, good["d_flux"], good["d_mass"], stream) == VP_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_flux).all()) and bool(torch.isnan(d_mass).all())          # nothing was launched
    n0 = torch.cuda.memory_stats()["allocation.all.allocated"]
    for _ in range(20):
        assert call(st.h, good["d_in"], n_in, good["d_flux"], good["d_mass"], stream) == 0
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0
    st.close()
    want_flux, want_mass, bnd = TC.flux_reference(x, hop, "args")
    assert np.all(np.abs(d_flux.cpu().numpy() - want_flux) <= bnd) and np.all(np.abs(d_mass.cpu().numpy() - want_mass) <= bnd)
    T2 = 2048 + 5 * 512
    st2 = StftRoundTrip(2, T2, 2048, 512)
    with pytest.raises(VpError) as e:
        st2.onset_flux(torch.zeros((2, T2), dtype=torch.float32, device="cuda"))
    assert e.value.code == VP_ERR_GEOMETRY and "2048-point frames are not built" in str(e.value)
    st2.close()
