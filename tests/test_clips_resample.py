"""frad_clips_resample alone: scipy.signal.resample_poly's arithmetic on many ragged float64 spans, converted and written as
frad_clips_window_add writes its windows.

Legs, raw pointers and guard bytes as in test_clips_ola.py ("emu": the CPU interpreter build of the same kernel source, "gpu": the
MI355X), whose backends are imported.

Bounds.  The entry point sums T <= 2 * half // up + 1 products in ascending source order with one fma each; the numpy model
``window.clips_resample_host`` sums the same terms in the same order with a multiply and an add.  Each is a recursive sum of T
terms, whose error is at most (T + 1) * 2**-53 * sum|x_i h_i| to first order, so the two differ by at most
``2 * (T + 1) * 2**-53 * max_phase(sum|h|) * max|x|`` (MODEL bound, computed from the taps; a phase is the set of taps one output
row reads: every up-th).  scipy.signal.resample_poly sums the same products with its own taps (firwin) and in its own order: the
model bound plus ``T * dh * max|x|`` with dh = max|taps - firwin(...) * up|, asserted <= 1e-14.  An impulse is exact
(fma(1, h, 0) = h), a window is the same terms in the same order as the whole clip (array_equal in every format), and every
other format is frad_from_f64 of the float64 output byte for byte."""
import numpy as np
import pytest

from frad_python_amd.backend.pcmformat import ff_format_to_numpy_type, from_f64, pcm_dtype_code
from frad_python_amd.window import clips_resample_host, resample_rows, resample_taps
from test_clips_ola import FLOAT_FORMATS, GUARD, INT_FORMATS, be  # noqa: F401  (be: the fixture)

FORMATS = ("f64le", "s16le", "u8", "f32be")
RATIOS = [(1, 3), (3, 1), (2, 3), (7, 5), (160, 147), (147, 160)]
_taps = {}


def taps_on(be, up, down):
    if (be.name, up, down) not in _taps:
        _taps[be.name, up, down] = be.put(resample_taps(up, down))
    return _taps[be.name, up, down]


def call(be, src, C, up, down, fmt, tables, out, out_at, out_rows, flags=2):
    """The raw entry point.  ``tables``: src_off, src_row0, src_rows, out_row0, valid, dst_row (or None), out_off; ``out``: a uint8
    host array (guards included) that is uploaded, written from byte ``out_at`` on, and returned."""
    so, s0, sr, o0, va, dst, off = tables
    d_src = be.put(np.ascontiguousarray(src, np.float64)) if src is not None and np.size(src) else None
    d = [be.put(np.ascontiguousarray(a, t)) for a, t in ((so, np.int64), (s0, np.int64), (sr, np.int32), (o0, np.int64), (va, np.int32),
                                                         (off, np.int64))]
    d_dst = be.put(np.ascontiguousarray(dst, np.int64)) if dst is not None else None
    d_out = be.put(out)
    be.lib.clips_resample(be.ptr(d_src), be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), len(so), C, up, down, be.ptr(taps_on(be, up, down)),
                          10 * max(up, down), be.ptr(d[3]), be.ptr(d[4]), be.ptr(d_dst), pcm_dtype_code(fmt), flags, be.ptr(d_out) + out_at,
                          be.ptr(d[5]), out_rows, be.stream)
    return be.get(d_out)


def ragged(be, src, C, up, down, fmt, so, s0, sr, o0, va, misalign=0):
    """spans written one after the other (no dst_row, span = valid) -> (array [rows, C], out_off); the guards are checked"""
    dt = ff_format_to_numpy_type(fmt)
    off = np.zeros(len(so) + 1, np.int64)
    np.cumsum(va, out=off[1:])
    nb = int(off[-1]) * C * dt.itemsize
    raw = call(be, src, C, up, down, fmt, (so, s0, sr, o0, va, None, off), np.full(misalign + nb + GUARD, 0xA5, np.uint8), misalign,
               int(off[-1]))
    assert (raw[:misalign] == 0xA5).all() and (raw[misalign + nb:] == 0xA5).all(), "guard bytes were written"
    return np.frombuffer(raw[misalign:misalign + nb].tobytes(), dt).reshape(-1, C), off


def short_span(up, down):
    """a span shorter than the filter's reach in source rows (2 * half / up), but more than two rows"""
    return max(3, min(2 * 10 * max(up, down) // up - 1, 17))


def lengths(up, down):
    return (0, 1, 2, short_span(up, down), 200)


def whole_clips(rng, C, up, down, rows_list, amp=1.0):
    """clips of ``rows_list`` source rows, each a stream of its own from row 0, resampled whole -> (src, tables)"""
    parts, so, at = [np.full(3, np.nan)], [], 3               # the spans need not start the buffer
    for rows in rows_list:
        so.append(at)
        parts.append(rng.uniform(-amp, amp, rows * C))
        at += rows * C
    src = np.concatenate(parts + [np.full(2, np.nan)])
    sr = np.array(rows_list, np.int32)
    va = np.array([resample_rows(r, up, down) for r in rows_list], np.int32)
    return src, (np.array(so, np.int64), np.zeros(len(so), np.int64), sr, np.zeros(len(so), np.int64), va)


def model_bound(up, down, amp):
    h = resample_taps(up, down)
    half = 10 * max(up, down)
    T = 2 * half // up + 1
    phase = max(np.abs(h[p::up]).sum() for p in range(up))
    return 2 * (T + 1) * 2.0 ** -53 * phase * amp, T


# ---------------------------------------------------------------------------------------------------------- 1. impulse, exact
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("up,down", RATIOS)
def test_an_impulse_gives_the_taps_exactly(be, up, down, C):
    h = resample_taps(up, down)
    half = 10 * max(up, down)
    for rows in lengths(up, down):
        for far in (0, 1 << 33):                              # ... and with the span far along the stream: 64-bit positions
            if rows == 0 and far:
                continue
            i0 = rows // 3                                     # the impulse's row inside the span
            x = np.zeros((max(rows, 1), C))
            if rows:
                x[i0] = 1.0 + np.arange(C)                     # (1, 2, 3: products with a power of two or 3 * h, still one rounding)
            s0 = far
            n_first = max(0, -(-((s0 + i0) * up - half) // down) - 3) if rows else 0      # three rows before the support
            count = 2 * half // down + 8 if rows else 5
            got, _ = ragged(be, x[:rows], C, up, down, "f64le", [0], [s0], [rows], [n_first], [count])
            n = n_first + np.arange(count, dtype=np.int64)
            k = n * down - (s0 + i0) * up + half
            want = np.where((k >= 0) & (k <= 2 * half) & (rows > 0), h[np.clip(k, 0, 2 * half)], 0.0)
            want = want[:, None] * (1.0 + np.arange(C))[None, :]
            assert (want != 0).any() or rows == 0
            assert np.array_equal(got, want), (rows, far)


# ------------------------------------------------------------------------------------------------------- 2. windows, exact
def support(a, b, up, down, rows):
    half = 10 * max(up, down)
    lo = max(0, -(-(a * down - half) // up))
    hi = min(rows, ((b - 1) * down + half) // up + 1)
    return (lo, hi) if hi > lo else (0, 0)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("up,down,rows", [(2, 3, 40), (7, 5, 23), (1, 3, 70), (160, 147, 30)])
def test_every_window_of_a_small_clip_is_the_slice_of_the_whole_clip(be, fmt, C, up, down, rows):
    rng = np.random.default_rng(up + down + C)
    x = rng.uniform(-1.1, 1.1, (rows, C))
    total = resample_rows(rows, up, down)
    step = 1 if total <= 40 else 3
    wins = [(a, b) for a in range(0, total + 1, step) for b in sorted({a, a + 1, a + 2, (a + total) // 2, total}) if b >= a and b <= total]
    so, s0, sr, o0, va = [], [], [], [], []
    for a, b in wins:                                          # the source span: the window's full support, clipped to the clip
        lo, hi = support(a, b, up, down, rows)
        so.append(5 + lo * C); s0.append(lo); sr.append(hi - lo); o0.append(a); va.append(b - a)
    src = np.concatenate([np.full(5, np.nan), x.reshape(-1), np.full(4, np.nan)])
    isz = ff_format_to_numpy_type(fmt).itemsize
    for misalign in (0, isz, 3 * isz):
        whole, _ = ragged(be, src, C, up, down, fmt, [5], [0], [rows], [0], [total], misalign=misalign)
        got, off = ragged(be, src, C, up, down, fmt, so, s0, sr, o0, va, misalign=misalign)
        for w, (a, b) in enumerate(wins):
            assert got[off[w]:off[w + 1]].tobytes() == whole[a:b].tobytes(), (fmt, misalign, a, b)


# -------------------------------------------------------------------------------------------- 3. the model, and 4. scipy
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("up,down", RATIOS)
def test_float64_output_against_the_numpy_model_and_scipy(be, up, down, C):
    from scipy.signal import firwin, resample_poly
    rng = np.random.default_rng(11 * up + down + C)
    amp = 1.1
    rows_list = list(lengths(up, down)) + [1300]               # 1300 rows: more than one block, and tiles inside one clip
    src, (so, s0, sr, o0, va) = whole_clips(rng, C, up, down, rows_list, amp)
    got, off = ragged(be, src, C, up, down, "f64le", so, s0, sr, o0, va)
    want, woff = clips_resample_host(src, so, s0, sr, C, up, down, o0, va)
    assert np.array_equal(off, woff) and got.shape == want.shape
    bound, T = model_bound(up, down, amp)
    err = np.max(np.abs(got - want))
    half = 10 * max(up, down)
    dh = np.max(np.abs(resample_taps(up, down) - firwin(2 * half + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up))
    print(f"[model] {up}/{down} C={C}: max|got - model| = {err:.3e} (bound {bound:.3e}), T = {T}, dh = {dh:.3e}")
    assert err <= bound
    assert dh <= 1e-14
    for j, rows in enumerate(rows_list):
        if not rows:
            assert off[j + 1] == off[j]
            continue
        x = src[so[j]:so[j] + rows * C].reshape(rows, C)
        ref = resample_poly(x, up, down, axis=0)
        g = got[off[j]:off[j + 1]]
        assert g.shape == ref.shape, (rows, g.shape, ref.shape)
        e = np.max(np.abs(g - ref))
        print(f"[scipy] {up}/{down} C={C} rows={rows}: max|got - scipy| = {e:.3e} (bound {bound + T * dh * amp:.3e})")
        assert e <= bound + T * dh * amp, rows


def test_a_tile_whose_source_rows_do_not_fit_in_lds_reads_them_from_global_memory(be):
    """1/40 with three channels: the 512 float64 stores of a tile read about 7 700 source rows of 24 bytes, more than the 48 KiB a
    block stages, so the whole clip takes the global-memory path; its short windows are staged.  Both paths run the same loop: a
    window is still the slice of the whole clip byte for byte, and the whole clip is within the model's bound."""
    up, down, C, rows = 1, 40, 3, 9000
    x = np.random.default_rng(40).uniform(-1.1, 1.1, (rows, C))
    total = resample_rows(rows, up, down)
    whole, _ = ragged(be, x, C, up, down, "f64le", [0], [0], [rows], [0], [total])
    want, _ = clips_resample_host(x, [0], [0], [rows], C, up, down, [0], [total])
    assert np.max(np.abs(whole - want)) <= model_bound(up, down, 1.1)[0]
    wins = [(0, 4), (100, 107), (total - 5, total)]
    so, s0, sr, o0, va = (np.array(v) for v in zip(*[(support(a, b, up, down, rows)[0] * C, support(a, b, up, down, rows)[0],
                                                      support(a, b, up, down, rows)[1] - support(a, b, up, down, rows)[0], a, b - a)
                                                     for a, b in wins]))
    for j in range(len(wins)):                                 # one launch each: the tile lies inside one clip and is staged
        got, _ = ragged(be, x, C, up, down, "f64le", so[j:j + 1], s0[j:j + 1], sr[j:j + 1], o0[j:j + 1], va[j:j + 1])
        assert got.tobytes() == whole[wins[j][0]:wins[j][1]].tobytes(), wins[j]


# ---------------------------------------------------------------------------------------------------------- 5. other formats
@pytest.mark.parametrize("up,down,C", [(2, 3, 3), (160, 147, 1), (3, 1, 2)])
def test_every_other_format_is_from_f64_of_the_float64_output(be, up, down, C):
    rng = np.random.default_rng(up + C)
    src, (so, s0, sr, o0, va) = whole_clips(rng, C, up, down, [0, 1, 2, 19, 200], amp=1.2)      # some samples overshoot +-1
    f64, off = ragged(be, src, C, up, down, "f64le", so, s0, sr, o0, va)
    flat = be.put(np.ascontiguousarray(f64.reshape(-1)))
    for fmt in INT_FORMATS + FLOAT_FORMATS:
        for flags in (2, 0):
            got = np.frombuffer(call(be, src, C, up, down, fmt, (so, s0, sr, o0, va, None, off),
                                     np.zeros(f64.size * ff_format_to_numpy_type(fmt).itemsize + 16, np.uint8), 0, int(off[-1]), flags).tobytes(),
                                np.uint8)[:f64.size * ff_format_to_numpy_type(fmt).itemsize]
            d_out = be.put(np.zeros(got.size + 16, np.uint8))
            be.lib.from_f64(be.ptr(flat), f64.size, pcm_dtype_code(fmt), be.ptr(d_out), be.stream, flags)
            assert got.tobytes() == be.get(d_out)[:got.size].tobytes(), (fmt, flags)


# ------------------------------------------------------------------------------------------------ 6. padding and scatter
@pytest.mark.parametrize("fmt,C,T,misalign", [("u8", 3, 37, 1), ("s16le", 2, 40, 0), ("f64le", 1, 33, 8), ("f32be", 2, 36, 0)])
def test_padding_is_silence_and_scatter_leaves_the_rest_alone(be, fmt, C, T, misalign):
    """valid below the span, dst_row in shuffled order, spans at odd addresses (u8, C = 3, out + 1) and at 16-byte aligned ones
    (s16le: T * C * 2 = 160): the padding is the conversion of 0.0, the batch rows no clip owns and the guards keep their bytes"""
    rng = np.random.default_rng(T)
    up, down, rows = 2, 3, 60
    x = rng.uniform(-1.1, 1.1, (rows, C))
    total = resample_rows(rows, up, down)
    wins = [(a, a + n) for a in range(0, total + 1, 5) for n in (0, 1, 5, 13, T) if a + n <= total]
    so, s0, sr, o0, va = (np.array(v) for v in zip(*[(support(a, b, up, down, rows)[0] * C, support(a, b, up, down, rows)[0],
                                                      support(a, b, up, down, rows)[1] - support(a, b, up, down, rows)[0], a, b - a)
                                                     for a, b in wins]))
    n = len(wins)
    B = n + 5                                                  # five batch rows belong to nobody
    dst = rng.permutation(B)[:n].astype(np.int64) * T
    off = np.arange(n + 1, dtype=np.int64) * T
    dt = ff_format_to_numpy_type(fmt)
    nb = B * T * C * dt.itemsize
    raw = call(be, x, C, up, down, fmt, (so, s0, sr, o0, va, dst, off), np.full(misalign + nb + GUARD, 0xA5, np.uint8), misalign, n * T)
    assert (raw[:misalign] == 0xA5).all() and (raw[misalign + nb:] == 0xA5).all(), "guard bytes were written"
    got = np.frombuffer(raw[misalign:misalign + nb].tobytes(), dt).reshape(B, T, C)
    want, woff = ragged(be, x, C, up, down, fmt, so, s0, sr, o0, va)
    silence = from_f64(np.zeros(1), fmt)[0]
    owned = np.zeros(B, bool)
    for w in range(n):
        row = got[dst[w] // T]
        owned[dst[w] // T] = True
        assert row[:va[w]].tobytes() == want[woff[w]:woff[w + 1]].tobytes(), (w, o0[w], va[w])
        assert (row[va[w]:] == silence).all() and row[va[w]:].tobytes() == np.full((T - va[w], C), silence, dt).tobytes(), w
    assert owned.sum() == n and (va == T).any() and (va == 0).any()
    assert (got[~owned].view(np.uint8) == 0xA5).all(), "a batch row outside the spans was written"
    # the same spans without dst_row: padded rows one after the other
    raw = call(be, x, C, up, down, fmt, (so, s0, sr, o0, va, None, off), np.full(misalign + n * T * C * dt.itemsize + GUARD, 0xA5, np.uint8),
               misalign, n * T)
    dense = np.frombuffer(raw[misalign:misalign + n * T * C * dt.itemsize].tobytes(), dt).reshape(n, T, C)
    assert dense.tobytes() == got[dst // T].tobytes()
    assert (raw[misalign + n * T * C * dt.itemsize:] == 0xA5).all()


# ---------------------------------------------------------------------------------------------------------- 7. status codes
def test_status_codes(be):
    from frad_python_amd._lib import FradError
    z = be.put(np.zeros(64, np.int64))
    p = be.ptr(z)
    tp = be.ptr(taps_on(be, 2, 3))
    args = lambda C=2, up=2, down=3, half=30, code=22, n=1, rows=1, **nul: (
        nul.get("src", p), nul.get("src_off", p), nul.get("src_row0", p), nul.get("src_rows", p), n, C, up, down, nul.get("taps", tp), half,
        nul.get("out_row0", p), nul.get("valid", p), 0, code, 2, nul.get("out", p), nul.get("out_off", p), rows, be.stream)
    for bad in (dict(C=0), dict(C=-1), dict(up=0), dict(down=0), dict(up=-2), dict(half=20), dict(half=31), dict(half=0), dict(up=3, half=20),
                dict(code=16), dict(code=24), dict(code=-1), dict(n=-1), dict(rows=-1), dict(src_off=0), dict(src_row0=0), dict(src_rows=0),
                dict(taps=0), dict(out_row0=0), dict(valid=0), dict(out=0), dict(out_off=0)):
        with pytest.raises(FradError) as e:
            be.lib.clips_resample(*args(**bad))
        assert e.value.status == -1, bad                       # FRAD_E_INVALID
    assert be.lib.clips_resample(*args(n=0, src_off=0, out=0)) is None      # nothing to do: no table is read, nothing is launched
    assert be.lib.clips_resample(*args(rows=0, src_off=0, out=0)) is None
    assert be.lib.clips_resample(*args()) is None              # all-zero tables: one clip without rows, an empty span
    assert be.lib.clips_resample(*args(src=0)) is None         # ... which reads no source


@pytest.mark.gpu
def test_core_wrapper_checks_the_tables_before_it_launches():
    """core.clips_resample: what the C-ABI cannot check (the tables live in device memory) is checked on the host."""
    import torch
    from frad_python_amd import core
    C, up, down = 2, 2, 3
    x = np.random.default_rng(3).uniform(-1, 1, (60, C))
    src = torch.from_numpy(x.reshape(-1)).to("cuda:0")
    taps = torch.from_numpy(resample_taps(up, down)).to("cuda:0")
    good = dict(src=src, src_off=[0, 20], src_row0=[0, 10], src_rows=[60, 50], out_row0=[0, 20], valid=[40, 10], span=None, dst_row=None,
                out=None, taps=taps)
    run = lambda kw: core.clips_resample(kw["src"], kw["src_off"], kw["src_row0"], kw["src_rows"], kw.get("C", C), kw.get("up", up),
                                         kw.get("down", down), kw["taps"], kw["out_row0"], kw["valid"], kw.get("fmt"), kw["span"],
                                         kw["dst_row"], kw["out"])
    out, off = run(good)
    assert off.tolist() == [0, 40, 50] and tuple(out.shape) == (50, C)
    want, _ = clips_resample_host(x, good["src_off"], good["src_row0"], good["src_rows"], C, up, down, good["out_row0"], good["valid"])
    assert np.max(np.abs(out.cpu().numpy() - want)) <= model_bound(up, down, 1.0)[0]
    batch = torch.zeros((4, 50, C), dtype=torch.float64, device="cuda:0")
    scatter = dict(good, span=[50, 50], dst_row=[150, 0], out=batch)
    assert run(scatter)[0] is batch
    for bad in (dict(src_off=[0, 21]), dict(src_off=[-1, 20]), dict(src_rows=[61, 50]), dict(src_rows=[60, -1]), dict(src_row0=[-1, 10]),
                dict(out_row0=[-1, 20]), dict(valid=[40, -1]), dict(valid=[40]), dict(src_off=[0]), dict(span=[39, 10]), dict(C=0), dict(up=0),
                dict(down=0), dict(up=4), dict(down=4), dict(taps=taps[:-1]), dict(fmt="s17le"), dict(out=batch), dict(src=None)):
        with pytest.raises(ValueError):
            run(dict(good, **bad))
            print("no ValueError for", {k: v for k, v in bad.items() if k not in ("taps", "out", "src")})
    for bad in (dict(dst_row=[150, 151]), dict(dst_row=[0, 49]), dict(dst_row=[151, 0]), dict(dst_row=[-1, 60]), dict(span=[39, 50]),
                dict(valid=[51, 10]), dict(dst_row=[0]), dict(out=None)):
        with pytest.raises(ValueError):
            run(dict(scatter, **bad))
            print("no ValueError for", {k: v for k, v in bad.items() if k != "out"})
