"""Channel-pointer entry points (vp_process_block_channels, vp_process_block_channels_device, vp_process_blocks_channels_device) against
the packed entry points, on twin handles with identical settings: one is fed the packed slab, the other the same samples through
pointer tables.  The channel path runs the same plans on the same values, so every comparison is BIT IDENTITY; each test also checks
that what it compared is a signal (rms behind the latency above 0.01).

Rows: every row its own allocation; stream 1's rows start one float into their allocation (no 16-byte alignment: the dword loop of
vp_k_gather_channels / vp_k_scatter_channels), stream 2 has no side chain (both pointers null), stream 3 lacks channel 1 only; the
packed twin holds zeros there (MyBuffer.cpp:93-102).  N = 441 is odd (dword accesses on every row), N = 100 and 256 allow 16-byte
accesses.  Every device output row sits between guard floats that must come back untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 44100.0
S = 5
CALLS = 12
NULL_IN = {(2, 1), (2, 2), (3, 1)}           # (stream, channel) without an input pointer
MISALIGNED = {1}                             # streams whose rows start one float into their allocation
GUARD = 8                                    # floats in front of and behind every device output row
SENTINEL = 1234.5


@functools.lru_cache(maxsize=None)
def _signal(T):
    """[S][3][T] float32 (CPU tensor), the null rows' samples zeroed: what the packed twin is fed.  Computed once per length."""
    from vocoderproject_amd.synth import make_streams
    x = make_streams(S, T).clone()
    for s, ch in NULL_IN:
        x[s, ch] = 0
    return x


def _proc(N, iir="exact", pitch=1, voc=1, path=None, reserve=0):
    from vocoderproject_amd import BatchVocoderProcessor
    p = BatchVocoderProcessor(pitchBool=pitch, vocBool=voc)
    p.prepareToPlay(FS, N, S)
    p.set_iir_mode(iir)
    if path:
        p.set_vocoder_path(path)
    if reserve:
        p.reserve_blocks(reserve)
    return p


def _row(L, s, fill=0.0):
    """A device row of L floats in an allocation of its own, with GUARD floats on either side; (allocation, row view)."""
    import torch
    off = GUARD + (1 if s in MISALIGNED else 0)
    base = torch.full((off + L + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    row = base[off:off + L]
    row.fill_(fill)
    assert (row.data_ptr() % 16 != 0) == (s in MISALIGNED)
    return base, row


def _guards_ok(base, row):
    import torch
    off = (row.data_ptr() - base.data_ptr()) // 4
    return bool(torch.all(base[:off] == SENTINEL)) and bool(torch.all(base[off + row.numel():] == SENTINEL))


def _in_rows(n_in, L):
    return [None if (s, ch) in NULL_IN else _row(L, s) for s in range(S) for ch in range(n_in)]


def _load(rows, n_in, x):
    """x [S][3][L] (device) into the non-null rows"""
    for s in range(S):
        for ch in range(n_in):
            r = rows[s * n_in + ch]
            if r is not None:
                r[1].copy_(x[s, ch])


def _rms_behind_latency(y, latency):
    """y [S][2][T]"""
    t = np.asarray(y, dtype=np.float64)[:, :, latency:]
    assert t.shape[2] > 0
    return float(np.sqrt(np.mean(t * t)))


@functools.lru_cache(maxsize=None)
def _packed_reference(N, iir, pitch, voc, mono=False):
    """The packed twin's output over CALLS single-block device calls: ([S][2][CALLS * N] numpy, latency).  Shared by the cases of a config."""
    import torch
    p = _proc(N, iir, pitch, voc)
    x = _signal(CALLS * N).cuda()
    y = torch.empty((CALLS, S, 2, N), dtype=torch.float32, device="cuda")
    for k in range(CALLS):
        blk = x[:, :, k * N:(k + 1) * N].contiguous()
        if mono:
            p.process_mono_device(blk[:, 0].contiguous(), y[k])
        else:
            p.process_device(blk, y[k])
    p.synchronize()
    lat = p.latency
    p.close()
    out = y.cpu().numpy().transpose(1, 2, 0, 3).reshape(S, 2, CALLS * N)
    out.setflags(write=False)
    return out, lat


CONFIGS = [(100, "exact", 1, 1), (256, "exact", 1, 1), (441, "exact", 1, 1), (256, "fast", 1, 0)]


@pytest.mark.parametrize("out_case", ["lr", "lr0_nan_prefill", "one_null_output"])
@pytest.mark.parametrize("N,iir,pitch,voc", CONFIGS)
def test_single_block_device_tables_match_the_packed_slab(N, iir, pitch, voc, out_case):
    import torch
    from vocoderproject_amd import BatchVocoderProcessor
    want, lat = _packed_reference(N, iir, pitch, voc)
    n_out = 2 if out_case == "lr" else 3
    null_out = {(4, 1)} if out_case == "one_null_output" else set()
    p = _proc(N, iir, pitch, voc)
    x = _signal(CALLS * N).cuda()
    ins = _in_rows(3, N)
    outs = [None if (s, ch) in null_out else _row(N, s, fill=float("nan")) for s in range(S) for ch in range(n_out)]
    guard = torch.full((N + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")       # what a write through a null entry might hit
    t_in = BatchVocoderProcessor.channel_table([r and r[1] for r in ins])
    t_out = BatchVocoderProcessor.channel_table([r and r[1] for r in outs])
    got = np.zeros((S, 2, CALLS * N), np.float32)
    for k in range(CALLS):
        _load(ins, 3, x[:, :, k * N:(k + 1) * N])
        for r in outs:
            if r is not None:
                r[1].fill_(float("nan"))
        p.process_channels_device(t_in, 3, t_out, n_out)
        for s in range(S):
            for ch in range(n_out):
                r = outs[s * n_out + ch]
                if r is None:
                    continue
                v = r[1].cpu().numpy()
                if ch < 2:
                    got[s, ch, k * N:(k + 1) * N] = v
                else:
                    assert np.array_equal(v, np.zeros(N, np.float32)), (k, s)            # MyBuffer.cpp:115: exactly 0 over the NaN prefill
    p.synchronize()
    for s in range(S):
        for ch in range(2):
            if (s, ch) in null_out:
                continue
            assert np.array_equal(got[s, ch], want[s, ch]), (s, ch, np.flatnonzero(got[s, ch] != want[s, ch])[:4])
    for r in outs:
        assert r is None or _guards_ok(*r)
    assert bool(torch.all(guard == SENTINEL))
    rms = _rms_behind_latency(want, lat)
    print(f"rms behind the latency: {rms:.4f}")
    assert rms > 0.01
    p.close()


def test_voice_only_tables_match_the_mono_entry_point():
    import torch  # noqa: F401
    from vocoderproject_amd import BatchVocoderProcessor
    N = 256
    want, lat = _packed_reference(N, "exact", 1, 1, True)
    p = _proc(N)
    x = _signal(CALLS * N).cuda()
    ins = [_row(N, s) for s in range(S)]
    outs = [_row(N, s) for s in range(S) for ch in range(2)]
    t_in = BatchVocoderProcessor.channel_table([r[1] for r in ins])
    t_out = BatchVocoderProcessor.channel_table([r[1] for r in outs])
    got = np.zeros((S, 2, CALLS * N), np.float32)
    for k in range(CALLS):
        _load(ins, 1, x[:, :, k * N:(k + 1) * N])
        p.process_channels_device(t_in, 1, t_out, 2)
        for i, r in enumerate(outs):
            got[i // 2, i % 2, k * N:(k + 1) * N] = r[1].cpu().numpy()
    p.synchronize()
    assert np.array_equal(got, want)
    assert all(_guards_ok(*r) for r in outs)
    assert _rms_behind_latency(want, lat) > 0.01
    p.close()


def _inplace_reference(N):
    """vp_process_block_inplace on the packed twin: [CALLS][S][3][N]"""
    p = _proc(N)
    x = _signal(CALLS * N).numpy()
    out = []
    for k in range(CALLS):
        io = np.ascontiguousarray(x[:, :, k * N:(k + 1) * N])
        p.processBlock(io)
        out.append(io)
    lat = p.latency
    p.close()
    return np.stack(out), lat


def test_in_place_tables_device_and_host_match_process_block_inplace():
    """Output entries equal to the input entries (JUCE's in-place buffer), n_in = n_out = 3: every input row is consumed before any output
    row is written.  A null entry is silence on the way in and "not wanted" on the way out."""
    from vocoderproject_amd import BatchVocoderProcessor
    N = 256
    want, lat = _inplace_reference(N)
    assert not want[:, :, 2].any()
    x = _signal(CALLS * N)
    # device
    p = _proc(N)
    xd = x.cuda()
    rows = _in_rows(3, N)
    table = BatchVocoderProcessor.channel_table([r and r[1] for r in rows])
    for k in range(CALLS):
        _load(rows, 3, xd[:, :, k * N:(k + 1) * N])
        p.process_channels_device(table, 3, table, 3)
        for i, r in enumerate(rows):
            if r is not None:
                assert np.array_equal(r[1].cpu().numpy(), want[k, i // 3, i % 3]), (k, i)
    p.synchronize()
    assert all(r is None or _guards_ok(*r) for r in rows)
    p.close()
    # host
    p = _proc(N)
    xn = x.numpy()
    for k in range(CALLS):
        hrows = [None if (s, ch) in NULL_IN else xn[s, ch, k * N:(k + 1) * N].copy() for s in range(S) for ch in range(3)]
        p.process_channels(hrows, hrows)
        for i, r in enumerate(hrows):
            if r is not None:
                assert np.array_equal(r, want[k, i // 3, i % 3]), (k, i)
    p.close()
    assert _rms_behind_latency(want[:, :, :2].transpose(1, 2, 0, 3).reshape(S, 2, CALLS * N), lat) > 0.01


@pytest.mark.parametrize("iir,pitch,voc,path,reserve", [("exact", 1, 0, None, 4), ("exact", 1, 0, None, 0), ("fast", 1, 1, "batched", 4)],
                         ids=["pitch_reserved", "pitch_unreserved", "both_fast_batched_reserved"])
def test_multi_block_tables_match_process_blocks_device(iir, pitch, voc, path, reserve):
    """Rows of n_blocks * N samples -- a stream's recording as it lies in memory -- against vp_process_blocks_device on the
    [n_blocks][S][3][N] slab.  Pitch only: the wave-specialised multi-block launch; both processes, VP_IIR_FAST, batched vocoder, reserved:
    the combined plan, whose rounding depends on how the blocks are grouped -- the twin must be grouped identically."""
    import torch
    from vocoderproject_amd import BatchVocoderProcessor
    N, B, calls = 256, 4, 3
    twin = _proc(N, iir, pitch, voc, path, reserve)
    p = _proc(N, iir, pitch, voc, path, reserve)
    if pitch and not voc:
        assert "ws" in p.pitch_kernel_name()
    x = _signal(calls * B * N).cuda()
    ins = _in_rows(3, B * N)
    outs = [_row(B * N, s, fill=float("nan")) for s in range(S) for ch in range(3)]
    t_in = BatchVocoderProcessor.channel_table([r and r[1] for r in ins])
    t_out = BatchVocoderProcessor.channel_table([r[1] for r in outs])
    n0 = p.alloc_count()
    want_all = []
    for k in range(calls):
        seg = x[:, :, k * B * N:(k + 1) * B * N]
        slab = seg.reshape(S, 3, B, N).permute(2, 0, 1, 3).contiguous()
        want = torch.empty((B, S, 2, N), dtype=torch.float32, device="cuda")
        assert twin.L.vp_process_blocks_device(twin.h, slab.data_ptr(), want.data_ptr(), B, None) == 0      # (raw: the mirror's method would reserve)
        _load(ins, 3, seg)
        for r in outs:
            r[1].fill_(float("nan"))
        p.process_channels_device(t_in, 3, t_out, 3, n_blocks=B)
        torch.cuda.synchronize()
        w = want.permute(1, 2, 0, 3).reshape(S, 2, B * N)
        for s in range(S):
            assert torch.equal(outs[s * 3][1], w[s, 0]) and torch.equal(outs[s * 3 + 1][1], w[s, 1]), (k, s)
            assert torch.equal(outs[s * 3 + 2][1], torch.zeros(B * N, device="cuda")), (k, s)
        want_all.append(w.cpu().numpy())
    assert p.alloc_count() == n0 and p.L.vp_get_reserved_blocks(p.h) == reserve
    twin.synchronize()
    p.synchronize()
    assert all(_guards_ok(*r) for r in outs)
    assert _rms_behind_latency(np.concatenate(want_all, axis=2), p.latency) > 0.01
    twin.close()
    p.close()


def test_host_rows_match_process_block_and_the_mono_path():
    N = 256
    x = _signal(CALLS * N).numpy()
    twin, p = _proc(N), _proc(N)
    twin_m, p_m = _proc(N), _proc(N)
    want_all = []
    for k in range(CALLS):
        blk = np.ascontiguousarray(x[:, :, k * N:(k + 1) * N])
        want = twin.process(blk)
        ins = [None if (s, ch) in NULL_IN else blk[s, ch].copy() for s in range(S) for ch in range(3)]
        outs = [np.full(N, np.nan, np.float32) for _ in range(S * 3)]
        outs[4 * 3 + 1] = None                                                  # one channel not wanted
        p.process_channels(ins, outs)
        for s in range(S):
            assert np.array_equal(outs[s * 3], want[s, 0]), (k, s)
            assert outs[s * 3 + 1] is None or np.array_equal(outs[s * 3 + 1], want[s, 1]), (k, s)
            assert np.array_equal(outs[s * 3 + 2], np.zeros(N, np.float32)), (k, s)
        want_all.append(want)
        # every side chain null: the mono path
        want_m = twin_m.process_mono(np.ascontiguousarray(blk[:, 0]))
        ins = [blk[s, 0].copy() if ch == 0 else None for s in range(S) for ch in range(3)]
        outs = [np.full(N, np.nan, np.float32) for _ in range(S * 2)]
        p_m.process_channels(ins, outs)
        assert np.array_equal(np.stack(outs).reshape(S, 2, N), want_m), k
    want = np.stack(want_all).transpose(1, 2, 0, 3).reshape(S, 2, CALLS * N)
    assert _rms_behind_latency(want, p.latency) > 0.01
    for q in (twin, p, twin_m, p_m):
        q.close()


def test_no_allocation_in_channel_calls_and_no_hidden_null_stream():
    """vp_debug_alloc_count is constant across channel calls, single and multi-block; and the device form issued on a non-default stream,
    its rows produced by a kernel queued on that stream just before, gives the packed twin's bits: nothing in the path runs on the
    null stream (it would read the rows before they are written, or scatter before the plan has run)."""
    import torch
    from vocoderproject_amd import BatchVocoderProcessor
    N, B = 256, 4
    T = 6 * N + 6 * B * N
    x = _signal(T).cuda()
    twin = _proc(N, "exact", 1, 0, None, B)
    p = _proc(N, "exact", 1, 0, None, B)
    n0 = p.alloc_count()
    st = torch.cuda.Stream()
    ins1, outs1 = _in_rows(3, N), [_row(N, s) for s in range(S) for ch in range(2)]
    insB, outsB = _in_rows(3, B * N), [_row(B * N, s) for s in range(S) for ch in range(2)]
    tabs = {1: (BatchVocoderProcessor.channel_table([r and r[1] for r in ins1]), BatchVocoderProcessor.channel_table([r[1] for r in outs1])),
            B: (BatchVocoderProcessor.channel_table([r and r[1] for r in insB]), BatchVocoderProcessor.channel_table([r[1] for r in outsB]))}
    busy = torch.randn(1024, 1024, device="cuda")
    torch.cuda.synchronize()
    t, wants = 0, []
    for nb, ins, outs in [(1, ins1, outs1)] * 6 + [(B, insB, outsB)] * 6:
        seg = x[:, :, t:t + nb * N]
        t += nb * N
        want = torch.empty((nb, S, 2, N), dtype=torch.float32, device="cuda")
        slab = seg.reshape(S, 3, nb, N).permute(2, 0, 1, 3).contiguous()
        assert twin.L.vp_process_blocks_device(twin.h, slab.data_ptr(), want.data_ptr(), nb, None) == 0
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            busy = busy @ busy * 1e-3                                           # work in front of the rows' producer on the same stream
            _load(ins, 3, seg)                                                  # the rows' producer: copy kernels on `st`
            p.process_channels_device(tabs[nb][0], 3, tabs[nb][1], 2, n_blocks=nb)    # (stream=None: the current torch stream, `st`)
        st.synchronize()
        w = want.permute(1, 2, 0, 3).reshape(S, 2, nb * N)
        for s in range(S):
            assert torch.equal(outs[s * 2][1], w[s, 0]) and torch.equal(outs[s * 2 + 1][1], w[s, 1]), (nb, s)
        wants.append(w.cpu().numpy())
    assert p.alloc_count() == n0
    p.synchronize()
    assert _rms_behind_latency(np.concatenate(wants, axis=2), p.latency) > 0.01
    twin.close()
    p.close()


def test_argument_errors_before_the_device_is_touched():
    from vocoderproject_amd import BatchVocoderProcessor
    p = BatchVocoderProcessor()
    L, h = p.L, p.h
    tab = (C.c_void_p * 16)()
    # not prepared
    assert L.vp_process_block_channels(h, tab, 3, tab, 3) == -2
    assert L.vp_process_block_channels_device(h, tab, 3, tab, 3, None) == -2
    assert L.vp_process_blocks_channels_device(h, tab, 3, tab, 3, 1, None) == -2
    p.prepareToPlay(FS, 64, 2)
    n0 = p.alloc_count()
    for n_in, n_out in [(2, 2), (0, 2), (4, 3), (3, 1), (3, 4), (1, 0)]:
        assert L.vp_process_block_channels(h, tab, n_in, tab, n_out) == -1
        assert L.vp_process_block_channels_device(h, tab, n_in, tab, n_out, None) == -1
        assert L.vp_process_blocks_channels_device(h, tab, n_in, tab, n_out, 1, None) == -1
    for n_blocks in (0, -3):
        assert L.vp_process_blocks_channels_device(h, tab, 3, tab, 3, n_blocks, None) == -1
    for a, b in [(None, tab), (tab, None)]:
        assert L.vp_process_block_channels(h, a, 3, b, 3) == -1
        assert L.vp_process_block_channels_device(h, a, 3, b, 3, None) == -1
        assert L.vp_process_blocks_channels_device(h, a, 3, b, 3, 2, None) == -1
    assert p.alloc_count() == n0
    # the handle is still good: an all-null host call is a block of silence
    outs = [np.full(64, np.nan, np.float32) for _ in range(2 * 3)]
    p.process_channels([None] * 6, outs)
    assert all(np.array_equal(o, np.zeros(64, np.float32)) for o in outs)
    p.close()
