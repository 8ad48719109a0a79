"""frad_clips_window_add alone: frad_clips_overlap_add's arithmetic on a row range of every clip, zero-padded and scattered.

Legs, raw pointers and guard bytes as in test_clips_ola.py ("emu": the CPU interpreter build of the same kernel source, "gpu": the
MI355X), whose backends, layout generator and runner are imported.

Bounds.  A window is the same arithmetic on the same rows as the whole clip, so against the whole-clip output of the same build
(this entry point with skip = 0, and frad_clips_overlap_add itself) it is array_equal in every format.  Against the numpy model
``window.clips_window_host`` the float64 output may differ in the last bits of the Hann weights: 1e-12 * max(1, max|want|), the
bound test_clips_ola.py documents for the same comparison."""
import numpy as np
import pytest

from frad_python_amd.backend.pcmformat import ff_format_to_numpy_type, from_f64, pcm_dtype_code
from frad_python_amd.window import clips_window_host
from test_clips_ola import GUARD, be, hann, layout, make_clips, run as run_ola  # noqa: F401  (be: the fixture)

FORMATS = ("f64le", "s16le", "u8", "f32be")


def call(be, frames, flat, N, C, ratio, fmt, tables, out, out_at, out_rows, win=True, flags=2):
    """The raw entry point.  ``tables``: clip_f0, clip_m, tail_off, tail_rows, skip, valid, dst_row (or None), out_off; ``out``: a
    uint8 host array (guards included) that is uploaded, written from byte ``out_at`` on, and returned."""
    f0, m, to, tr, sk, va, dst, off = tables
    cut = N * (ratio - 1) // ratio if ratio else N
    d_frames = be.put(frames) if frames is not None and frames.size else None
    d_flat = be.put(flat) if flat is not None else None
    d = [be.put(np.ascontiguousarray(a, t)) for a, t in ((f0, np.int64), (m, np.int32), (to, np.int64), (tr, np.int32), (sk, np.int64),
                                                         (va, np.int32), (off, np.int64))]
    d_dst = be.put(np.ascontiguousarray(dst, np.int64)) if dst is not None else None
    d_win = be.put(hann(N - cut)) if win and ratio and N - cut else None
    d_out = be.put(out)
    be.lib.clips_window_add(be.ptr(d_frames), be.ptr(d[0]), be.ptr(d[1]), len(f0), N, C, ratio, be.ptr(d_flat), be.ptr(d[2]), be.ptr(d[3]),
                            be.ptr(d_win), be.ptr(d[4]), be.ptr(d[5]), be.ptr(d_dst), pcm_dtype_code(fmt), flags, be.ptr(d_out) + out_at,
                            be.ptr(d[6]), out_rows, be.stream)
    return be.get(d_out)


def ragged(be, frames, flat, N, C, ratio, fmt, f0, m, to, tr, sk, va, misalign=0):
    """windows written one after the other (no dst_row, span = valid) -> (array [rows, C], out_off); the guards are checked"""
    dt = ff_format_to_numpy_type(fmt)
    off = np.zeros(len(f0) + 1, np.int64)
    np.cumsum(va, out=off[1:])
    nb = int(off[-1]) * C * dt.itemsize
    raw = call(be, frames, flat, N, C, ratio, fmt, (f0, m, to, tr, sk, va, None, off), np.full(misalign + nb + GUARD, 0xA5, np.uint8),
               misalign, int(off[-1]))
    assert (raw[:misalign] == 0xA5).all() and (raw[misalign + nb:] == 0xA5).all(), "guard bytes were written"
    return np.frombuffer(raw[misalign:misalign + nb].tobytes(), dt).reshape(-1, C), off


def timeline(m, tr, N, ratio):
    cut = N * (ratio - 1) // ratio if ratio else N
    return m * cut + (tr if tr else (N - cut if m else 0))


# ------------------------------------------------------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("N,C,ratio", [(128, 3, 16), (128, 2, 2), (128, 1, 0), (2240, 2, 3)])
def test_whole_clips_equal_frad_clips_overlap_add_byte_for_byte(be, N, C, ratio):
    rng = np.random.default_rng(N + 7 * C + ratio)
    clips = make_clips(rng, N, C, ratio, (0, 1, 2, 7), ("none", "L", "L+1", "N-1", "long"))
    clips = [clips[i] for i in rng.permutation(len(clips))]
    frames, cf, flat, tail_off, tail_rows, out_off = layout(clips, N, C, ratio)
    for fmt in FORMATS:
        for misalign in (0, 2 * ff_format_to_numpy_type(fmt).itemsize):
            want, off = run_ola(be, clips, N, C, ratio, fmt, misalign=misalign)
            got, off2 = ragged(be, frames, flat, N, C, ratio, fmt, cf[:-1], np.diff(cf), tail_off, tail_rows, np.zeros(len(clips), np.int64),
                               np.diff(out_off), misalign=misalign)
            assert np.array_equal(off, off2)
            assert got.tobytes() == want.tobytes(), (fmt, misalign)


# ------------------------------------------------------------------------------------- 2. every window of small clips
def small_clips(rng, N, C, shapes):
    """[(m, tail rows)] -> frames [sum m, N, C], flat tails, and per clip (f0, m, tail_off, tail_rows)"""
    frames = rng.uniform(-1.1, 1.1, (sum(m for m, _ in shapes), N, C))
    parts, clips, f0, at = [np.full(3, np.nan)], [], 0, 3
    for m, rows in shapes:
        clips.append((f0, m, at if rows else 0, rows))
        f0 += m
        if rows:
            parts.append(rng.uniform(-1.1, 1.1, rows * C))
            at += rows * C
    return frames, np.concatenate(parts + [np.full(2, np.nan)]), clips


def windows_of(clips, N, ratio, lengths=None):
    """every (start, length) of every clip as a window of its own (``lengths(rest)``: the lengths tried at a start) -> tables"""
    rows = []
    for j, (f0, m, to, tr) in enumerate(clips):
        T = timeline(m, tr, N, ratio)
        for start in range(T + 1):
            for n in (range(T - start + 1) if lengths is None else sorted({x for x in lengths(T - start) if 0 <= x <= T - start})):
                rows.append((f0, m, to, tr, start, n, j))
    return [np.array([r[i] for r in rows]) for i in range(7)]


def check_windows(be, rng, N, C, ratio, shapes, fmt, lengths=None):
    frames, flat, clips = small_clips(rng, N, C, shapes)
    whole_t = [np.array([c[i] for c in clips]) for i in range(4)]
    full = np.array([timeline(c[1], c[3], N, ratio) for c in clips])
    whole, woff = ragged(be, frames, flat, N, C, ratio, fmt, *whole_t, np.zeros(len(clips), np.int64), full)
    f0, m, to, tr, sk, va, which = windows_of(clips, N, ratio, lengths)
    got, off = ragged(be, frames, flat, N, C, ratio, fmt, f0, m, to, tr, sk, va)
    model = None
    if fmt == "f64le":
        tails_at0 = [flat]                                     # tail_off counts elements of the flat buffer as it is
        model, moff = clips_window_host(frames, f0, m, N, C, ratio, tails_at0, to, tr, sk, va)
        assert np.array_equal(moff, off)
    for w in range(len(f0)):
        g = got[off[w]:off[w + 1]]
        want = whole[woff[which[w]] + sk[w]:woff[which[w]] + sk[w] + va[w]]
        assert g.tobytes() == want.tobytes(), (fmt, C, which[w], sk[w], va[w])
        if model is not None and g.size:
            mw = model[off[w]:off[w + 1]]
            assert np.max(np.abs(g - mw)) <= 1e-12 * max(1.0, np.max(np.abs(mw))), (C, which[w], sk[w], va[w])
    return len(f0)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_window_of_a_small_clip_is_the_slice_of_the_whole_clip(be, fmt, C):
    n = check_windows(be, np.random.default_rng(5 + C), 16, C, 4, [(3, 10), (3, 0), (0, 10), (1, 0)], fmt)
    assert n == 47 * 48 // 2 + 41 * 42 // 2 + 11 * 12 // 2 + 17 * 18 // 2


@pytest.mark.parametrize("N,ratio", [(48, 0), (48, 2), (48, 3), (48, 16)])
def test_further_ratios(be, N, ratio):
    cut = N * (ratio - 1) // ratio if ratio else N
    L = N - cut
    some = lambda rest: (0, 1, L, L + 1, cut - 1, cut, cut + 1, rest - 1, rest)
    check_windows(be, np.random.default_rng(ratio), N, 2, ratio, [(3, L + 5), (2, 0), (0, N - 1), (1, max(L, 1))], "f64le", some)


# ------------------------------------------------------------------------------------------------ 3. padding and scatter
@pytest.mark.parametrize("fmt,C,T,misalign", [("u8", 3, 37, 1), ("s16le", 2, 40, 0), ("f64le", 1, 33, 8), ("f32be", 2, 36, 0)])
def test_padding_is_silence_and_scatter_leaves_the_rest_alone(be, fmt, C, T, misalign):
    """valid below the span, dst_row in shuffled order, spans at odd addresses (u8, C = 3, out + 1) and at 16-byte aligned ones
    (s16le: T * C * 2 = 160): the padding is the conversion of 0.0, the batch rows no clip owns and the guards keep their bytes"""
    rng = np.random.default_rng(T)
    N, ratio = 16, 4
    frames, flat, clips = small_clips(rng, N, C, [(3, 10), (3, 0), (0, 10), (1, 0)])
    f0, m, to, tr, sk, va, which = windows_of(clips, N, ratio, lambda rest: (0, 1, 5, 13, rest))
    keep = va <= T
    f0, m, to, tr, sk, va, which = (a[keep] for a in (f0, m, to, tr, sk, va, which))
    n = len(f0)
    B = n + 5                                                  # five batch rows belong to nobody
    dst = rng.permutation(B)[:n].astype(np.int64) * T
    off = np.arange(n + 1, dtype=np.int64) * T
    dt = ff_format_to_numpy_type(fmt)
    nb = B * T * C * dt.itemsize
    raw = call(be, frames, flat, N, C, ratio, fmt, (f0, m, to, tr, sk, va, dst, off), np.full(misalign + nb + GUARD, 0xA5, np.uint8), misalign,
               n * T)
    assert (raw[:misalign] == 0xA5).all() and (raw[misalign + nb:] == 0xA5).all(), "guard bytes were written"
    got = np.frombuffer(raw[misalign:misalign + nb].tobytes(), dt).reshape(B, T, C)
    want, woff = ragged(be, frames, flat, N, C, ratio, fmt, f0, m, to, tr, sk, va)
    silence = from_f64(np.zeros(1), fmt)[0]
    owned = np.zeros(B, bool)
    for w in range(n):
        row = got[dst[w] // T]
        owned[dst[w] // T] = True
        assert row[:va[w]].tobytes() == want[woff[w]:woff[w + 1]].tobytes(), (w, sk[w], va[w])
        assert (row[va[w]:] == silence).all() and row[va[w]:].tobytes() == np.full((T - va[w], C), silence, dt).tobytes(), w
    assert owned.sum() == n
    assert (got[~owned].view(np.uint8) == 0xA5).all(), "a batch row outside the spans was written"
    # the same spans without dst_row: padded rows one after the other
    raw = call(be, frames, flat, N, C, ratio, fmt, (f0, m, to, tr, sk, va, None, off), np.full(misalign + n * T * C * dt.itemsize + GUARD, 0xA5,
                                                                                                np.uint8), misalign, n * T)
    dense = np.frombuffer(raw[misalign:misalign + n * T * C * dt.itemsize].tobytes(), dt).reshape(n, T, C)
    assert dense.tobytes() == got[dst // T].tobytes()
    assert (raw[misalign + n * T * C * dt.itemsize:] == 0xA5).all()


# ---------------------------------------------------------------------------------------------------------- 4. status codes
def test_status_codes(be):
    from frad_python_amd._lib import FradError
    z = be.put(np.zeros(64, np.int64))
    p = be.ptr(z)
    args = lambda N=16, C=2, ratio=4, code=22, n=1, rows=1, **nul: (
        nul.get("frames", p), nul.get("clip_f0", p), nul.get("clip_m", p), n, N, C, ratio, nul.get("tails", p), nul.get("tail_off", p),
        nul.get("tail_rows", p), 0, nul.get("skip", p), nul.get("valid", p), 0, code, 2, nul.get("out", p), nul.get("out_off", p), rows, be.stream)
    for bad in (dict(N=0), dict(C=0), dict(ratio=1), dict(ratio=257), dict(ratio=-1), dict(code=16), dict(code=24), dict(n=-1), dict(rows=-1),
                dict(clip_f0=0), dict(clip_m=0), dict(tail_off=0), dict(tail_rows=0), dict(skip=0), dict(valid=0), dict(out=0), dict(out_off=0)):
        with pytest.raises(FradError) as e:
            be.lib.clips_window_add(*args(**bad))
        assert e.value.status == -1, bad                       # FRAD_E_INVALID
    assert be.lib.clips_window_add(*args(n=0, clip_f0=0, out=0)) is None       # nothing to do: no table is read, nothing is launched
    assert be.lib.clips_window_add(*args(rows=0, clip_f0=0, out=0)) is None
    assert be.lib.clips_window_add(*args()) is None            # all-zero tables: one clip without frames, an empty span


@pytest.mark.gpu
def test_core_wrapper_checks_the_tables_before_it_launches():
    """core.clips_window_add: what the C-ABI cannot check (the tables live in device memory) is checked on the host."""
    import torch
    from frad_python_amd import core
    N, C, ratio = 16, 2, 4
    frames = torch.zeros((3, N, C), dtype=torch.float64, device="cuda:0")
    tails = torch.zeros(10 * C, dtype=torch.float64, device="cuda:0")
    good = dict(frames=frames, clip_f0=[0, 1], clip_m=[3, 2], tails=tails, tail_off=[0, 0], tail_rows=[10, 0], skip=[5, 0], valid=[41, 28],
                span=None, dst_row=None, out=None)
    run = lambda kw: core.clips_window_add(kw["frames"], kw["clip_f0"], kw["clip_m"], N, C, kw.get("ratio", ratio), kw["tails"], kw["tail_off"],
                                           kw["tail_rows"], kw["skip"], kw["valid"], kw.get("fmt"), None, kw["span"], kw["dst_row"], kw["out"])
    out, off = run(good)
    assert off.tolist() == [0, 41, 69] and tuple(out.shape) == (69, C)
    batch = torch.zeros((4, 50, C), dtype=torch.float64, device="cuda:0")
    scatter = dict(good, span=[50, 50], dst_row=[150, 0], out=batch)
    assert run(scatter)[0] is batch
    for bad in (dict(clip_f0=[0, 2]), dict(clip_f0=[-1, 1]), dict(clip_m=[3, -1]), dict(clip_m=[4, 2]), dict(tail_rows=[3, 0]),
                dict(tail_rows=[11, 0]), dict(tail_off=[1, 0]), dict(tail_off=[-1, 0]), dict(skip=[6, 0]), dict(skip=[-1, 0]),
                dict(valid=[42, 28]), dict(valid=[41, 29]), dict(valid=[-1, 28]), dict(valid=[41]), dict(span=[40, 28]), dict(ratio=1),
                dict(ratio=300), dict(fmt="s17le"), dict(out=batch)):
        with pytest.raises(ValueError):
            run(dict(good, **bad))
    for bad in (dict(dst_row=[150, 151]), dict(dst_row=[0, 49]), dict(dst_row=[151, 0]), dict(dst_row=[-1, 60]), dict(span=[40, 50]),
                dict(dst_row=[0]), dict(out=None)):
        with pytest.raises(ValueError):
            run(dict(scatter, **bad))
