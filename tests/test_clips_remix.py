"""frad_clips_remix alone: a float64 matrix [C_out, C_in] applied to every row of many ragged float64 spans whose channel count
differs per clip, converted and written as frad_clips_window_add writes its windows.

Legs, raw pointers and guard bytes as in test_clips_ola.py ("emu": the CPU interpreter build of the same kernel source, "gpu": the
MI355X), whose backends are imported.

No tolerance anywhere.  The entry point's arithmetic is defined term by term (include/frad_hip.h): for an output channel the
terms are the source channels, ascending, whose weight is not 0.0; the first sets the sum, every later one is a rounded multiply
and a rounded add.  ``window.clips_remix_host`` is that definition in numpy, so the float64 output is array_equal to it for every
matrix, an identity or permutation row is the source's bits, and every other format is ``pcmformat.from_f64`` of the float64
output byte for byte.  (Sources with +-Inf meet selection matrices only: Inf - Inf is a NaN whose sign bit differs between an
x86 host and the device, and a NaN has no place in PCM.)"""
import os

import numpy as np
import pytest

from frad_python_amd.backend.pcmformat import ff_format_to_numpy_type, from_f64, pcm_dtype_code
from frad_python_amd.window import clips_remix_host
from test_clips_ola import FLOAT_FORMATS, GUARD, INT_FORMATS, be  # noqa: F401  (be: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIALS = np.array([0.0, -0.0, 5e-324, -2.2e-311, np.inf, -np.inf, 1e308, -1e308, 0.3, -1.7, 2.0 ** -1022, 1.0, -1.0, 0.1])
FINITE = SPECIALS[np.isfinite(SPECIALS)]


def layout(be, clips):
    """clips: [(x [rows, C_in] or None, M [C_out, C_in])] -> what has to stay alive, and the device tables: the sources lie in one
    buffer with NaNs between them (so a clip starts at 8 or at 16 bytes), a matrix that two clips share is placed once"""
    parts, at, where = [np.full(3, np.nan)], 3, []
    for x, _ in clips:
        where.append(at)
        if x is not None and x.size:
            parts.append(np.ascontiguousarray(x, np.float64).reshape(-1))
            at += x.size
            parts.append(np.full(1 + len(where) % 2, np.nan))
            at += parts[-1].size
    d_src = be.put(np.concatenate(parts))
    ptr = np.array([be.ptr(d_src) + 8 * w if x is not None and x.size else 0 for w, (x, _) in zip(where, clips)], np.int64)
    ch = np.array([m.shape[1] for _, m in clips], np.int32)
    placed, flat, mat_off, at = {}, [np.full(2, np.nan)], [], 2
    for _, m in clips:
        if id(m) not in placed:
            placed[id(m)] = at
            flat.append(np.ascontiguousarray(m, np.float64).reshape(-1))
            at += m.size
        mat_off.append(placed[id(m)])
    return d_src, be.put(ptr), be.put(ch), be.put(np.concatenate(flat)), be.put(np.array(mat_off, np.int64))


def call(be, clips, C_out, fmt, valid, dst, off, out, out_at, out_rows, flags=2):
    """The raw entry point.  ``out``: a uint8 host array (guards included) that is uploaded, written from byte ``out_at`` on, and
    returned."""
    keep = layout(be, clips)
    d_valid, d_off = be.put(np.ascontiguousarray(valid, np.int32)), be.put(np.ascontiguousarray(off, np.int64))
    d_dst = be.put(np.ascontiguousarray(dst, np.int64)) if dst is not None else None
    d_out = be.put(out)
    be.lib.clips_remix(be.ptr(keep[1]), be.ptr(keep[2]), be.ptr(keep[3]), be.ptr(keep[4]), len(clips), C_out, be.ptr(d_valid), be.ptr(d_dst),
                       pcm_dtype_code(fmt), flags, be.ptr(d_out) + out_at, be.ptr(d_off), out_rows, be.stream)
    got = be.get(d_out)
    del keep
    return got


def ragged(be, clips, C_out, fmt="f64le", misalign=0, flags=2):
    """spans written one after the other (no dst_row, span = valid = the clip's rows) -> (array [rows, C_out], out_off); the guards
    are checked"""
    dt = ff_format_to_numpy_type(fmt)
    valid = np.array([0 if x is None else len(x) for x, _ in clips], np.int32)
    off = np.zeros(len(clips) + 1, np.int64)
    np.cumsum(valid, out=off[1:])
    nb = int(off[-1]) * C_out * dt.itemsize
    raw = call(be, clips, C_out, fmt, valid, None, off, np.full(misalign + nb + GUARD, 0xA5, np.uint8), misalign, int(off[-1]), flags)
    assert (raw[:misalign] == 0xA5).all() and (raw[misalign + nb:] == 0xA5).all(), "guard bytes were written"
    return np.frombuffer(raw[misalign:misalign + nb].tobytes(), dt).reshape(-1, C_out), off


def model(clips, C_out):
    pieces = [clips_remix_host(x, m) for x, m in clips if x is not None]
    return np.concatenate(pieces) if pieces else np.zeros((0, C_out))


def special_rows(rows, C, seed, pool=SPECIALS):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (rows, C))
    pick = rng.random((rows, C)) < 0.6
    x[pick] = pool[rng.integers(0, len(pool), int(pick.sum()))]
    return x


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


ROWS = (0, 1, 2, 7, 200)


# ------------------------------------------------------------------------------------------------------ 1. special values, exact
@pytest.mark.parametrize("C_out", [1, 2, 3])
@pytest.mark.parametrize("C_in", [1, 2, 3, 5])
def test_selection_rows_copy_the_sources_bits_and_a_zero_row_is_plus_zero(be, C_in, C_out):
    rng = np.random.default_rng(10 * C_in + C_out)
    sel = rng.permutation(max(C_in, C_out))[:C_out] % C_in     # output channel k is source channel sel[k]: a permutation where
    pick = np.zeros((C_out, C_in))                             # C_in >= C_out, the identity's shape where they are equal
    pick[np.arange(C_out), sel] = 1.0
    eye = np.eye(C_out, C_in)                                  # (rows beyond C_in are all zero)
    zero_row = pick.copy()
    zero_row[C_out - 1] = 0.0
    for m, src_of in ((pick, sel), (eye, np.arange(C_out)), (zero_row, sel)):
        clips = [(special_rows(rows, C_in, rows + C_in), m) for rows in ROWS]
        got, off = ragged(be, clips, C_out)
        assert off[-1] == sum(ROWS) and not np.isnan(got).any(), "a zero weight next to an Inf gave a NaN"
        x = np.concatenate([c[0] for c in clips])
        assert np.isinf(x).any() and (bits(x) == bits(-0.0)).any() and (np.abs(x[x != 0]) < 2.0 ** -1022).any()
        for k in range(C_out):
            if not m[k].any():
                assert (bits(got[:, k]) == 0).all(), "an all-zero row gives +0.0"
            else:
                assert np.array_equal(bits(got[:, k]), bits(x[:, src_of[k]])), (k, m)
        assert np.array_equal(bits(got), bits(model(clips, C_out)))


# -------------------------------------------------------------------------------------------------------- 2. random matrices
WEIGHTS = np.array([0.5, 0.25, 1 / 3, 0.7071067811865476, -0.7071067811865476, -1 / 3, -0.5, 1.0, 0.0, 0.0])


def random_matrix(rng, C_out, C_in):
    return WEIGHTS[rng.integers(0, len(WEIGHTS), (C_out, C_in))]


@pytest.mark.parametrize("C_out", [1, 2, 3])
@pytest.mark.parametrize("C_in", [1, 2, 3, 5])
def test_float64_output_is_the_numpy_model_bit_for_bit(be, C_in, C_out):
    rng = np.random.default_rng(100 * C_in + C_out)
    for trial in range(3):
        m = random_matrix(rng, C_out, C_in)
        clips = [(special_rows(rows, C_in, rows + trial, FINITE), m) for rows in ROWS]
        got, _ = ragged(be, clips, C_out)
        want = model(clips, C_out)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), m
    dyadic = np.full((C_out, C_in), 0.5)
    dyadic[0, ::2] = 0.25
    clips = [(rng.uniform(-1, 1, (200, C_in)), dyadic)]
    assert np.array_equal(bits(ragged(be, clips, C_out)[0]), bits(model(clips, C_out)))


@pytest.mark.parametrize("C_in,C_out", [(2, 1), (1, 2), (3, 2), (5, 3), (2, 2)])
def test_every_other_format_is_from_f64_of_the_float64_output(be, C_in, C_out):
    rng = np.random.default_rng(C_in + 7 * C_out)
    m = random_matrix(rng, C_out, C_in)
    m[0, 0] = 0.7071067811865476
    gain = 1.0 / max(1.0, np.abs(m).sum(axis=1).max())
    clips = [(rng.uniform(-1.0, 1.0, (rows, C_in)) * gain, m) for rows in ROWS]
    f64, off = ragged(be, clips, C_out)
    assert np.array_equal(bits(f64), bits(model(clips, C_out))) and np.abs(f64).max() < 1.0
    for fmt in INT_FORMATS + FLOAT_FORMATS:
        dt = ff_format_to_numpy_type(fmt)
        want = from_f64(f64, fmt)
        for misalign in (0, dt.itemsize, 3 * dt.itemsize):
            got, goff = ragged(be, clips, C_out, fmt, misalign)
            assert np.array_equal(goff, off) and got.tobytes() == want.tobytes(), (fmt, misalign)
    # samples beyond +-1: what numpy's astype gives for them is the host's own (it differs between x86 instruction sets), so the
    # yardstick there is the library's conversion, frad_from_f64, of the float64 output -- with and without FRAD_RAW_BE_INTS
    loud = [(x * (1.3 / np.abs(f64).max()), mm) for x, mm in clips]
    f64, off = ragged(be, loud, C_out)
    assert np.array_equal(bits(f64), bits(model(loud, C_out))) and np.abs(f64).max() > 1.0
    flat = be.put(np.ascontiguousarray(f64.reshape(-1)))
    for fmt in INT_FORMATS + FLOAT_FORMATS:
        for flags in (2, 0):
            got, _ = ragged(be, loud, C_out, fmt, flags=flags)
            d_out = be.put(np.zeros(got.nbytes + 16, np.uint8))
            be.lib.from_f64(be.ptr(flat), f64.size, pcm_dtype_code(fmt), be.ptr(d_out), be.stream, flags)
            assert got.tobytes() == be.get(d_out)[:got.nbytes].tobytes(), (fmt, flags)


# --------------------------------------------------------------------------------------- 3. clips of different C_in in one launch
@pytest.mark.parametrize("fmt", ["f64le", "s16le", "u8"])
@pytest.mark.parametrize("C_out", [1, 2])
def test_one_launch_mixes_clips_of_different_channel_counts(be, C_out, fmt):
    rng = np.random.default_rng(C_out)
    shared = random_matrix(rng, C_out, 2)
    mono = random_matrix(rng, C_out, 1) + 0.125
    empty = (None, mono)
    x = lambda rows, C: special_rows(rows, C, rows + C, FINITE[np.abs(FINITE) <= 2]) * 0.4
    clips = [empty, (x(5, 1), mono), (x(7, 2), shared), empty, (x(200, 3), random_matrix(rng, C_out, 3)), (x(9, 2), shared),
             (x(2, 1), random_matrix(rng, C_out, 1)), (np.zeros((0, 5)), random_matrix(rng, C_out, 5)), empty]
    want = model(clips, C_out)
    got, off = ragged(be, clips, C_out, fmt)
    assert off.tolist() == [0, 0, 5, 12, 12, 212, 221, 223, 223, 223]
    assert got.tobytes() == from_f64(want, fmt).tobytes()
    for j, (xj, mj) in enumerate(clips):                       # ... which is the per-clip model
        if xj is not None:
            assert got[off[j]:off[j + 1]].tobytes() == from_f64(clips_remix_host(xj, mj), fmt).tobytes(), j


@pytest.mark.parametrize("fmt", ["f64le", "s16le"])
def test_a_launch_of_several_blocks(be, fmt):
    """6 000 rows of three channels: nine tiles of 2 048 float64 elements, three of 8 192 s16le ones, and clips that end inside a
    tile"""
    rng = np.random.default_rng(8)
    m2, m5 = random_matrix(rng, 3, 2), random_matrix(rng, 3, 5)
    clips = [(rng.uniform(-0.3, 0.3, (2501, 2)), m2), (None, m2), (rng.uniform(-0.3, 0.3, (2999, 5)), m5), (rng.uniform(-0.3, 0.3, (500, 2)), m2)]
    got, off = ragged(be, clips, 3, fmt, misalign=ff_format_to_numpy_type(fmt).itemsize)
    assert off[-1] == 6000 and got.tobytes() == from_f64(model(clips, 3), fmt).tobytes()


# ------------------------------------------------------------------------------------------------ 4. padding and scatter
@pytest.mark.parametrize("fmt,C_out,T,misalign", [("s16le", 1, 24, 0), ("s16le", 3, 7, 0), ("u8", 3, 37, 1), ("f64le", 2, 3, 0), ("f64le", 1, 5, 8),
                                                  ("f32be", 2, 6, 0), ("f32be", 1, 9, 0)])
def test_padding_is_silence_and_scatter_leaves_the_rest_alone(be, fmt, C_out, T, misalign):
    """valid below the span, dst_row in shuffled order, row pitches T * C_out * itemsize that are a multiple of 16 bytes (s16le:
    24 * 1 * 2 = 48; f64le: 48; f32be: 48) and that are not (s16le: 7 * 3 * 2 = 42; u8: 111 from out + 1; f64le from out + 8: 40;
    f32be: 36): the padding is the conversion of 0.0, the batch rows no clip owns and the guards keep their bytes"""
    rng = np.random.default_rng(T + C_out)
    chans = [1, 2, 3, 2, 1, 5, 2, 1, 3, 2, 1, 2]
    rows = [0, 1, T, T // 2, 2, T - 1, 0, T, 3, 1, T // 3, T]
    mats = {c: random_matrix(rng, C_out, c) for c in set(chans)}
    clips = [(rng.uniform(-1.1, 1.1, (r, c)) * 0.4 if r else None, mats[c]) for r, c in zip(rows, chans)]
    n = len(clips)
    B = n + 5                                                  # five batch rows belong to nobody
    dst = rng.permutation(B)[:n].astype(np.int64) * T
    off = np.arange(n + 1, dtype=np.int64) * T
    valid = np.array(rows, np.int32)
    dt = ff_format_to_numpy_type(fmt)
    nb = B * T * C_out * dt.itemsize
    raw = call(be, clips, C_out, fmt, valid, dst, off, np.full(misalign + nb + GUARD, 0xA5, np.uint8), misalign, n * T)
    assert (raw[:misalign] == 0xA5).all() and (raw[misalign + nb:] == 0xA5).all(), "guard bytes were written"
    got = np.frombuffer(raw[misalign:misalign + nb].tobytes(), dt).reshape(B, T, C_out)
    silence = from_f64(np.zeros(1), fmt)[0]
    if fmt == "u8":
        assert silence == 128
    owned = np.zeros(B, bool)
    for w, (x, m) in enumerate(clips):
        row = got[dst[w] // T]
        owned[dst[w] // T] = True
        if x is not None:
            assert row[:valid[w]].tobytes() == from_f64(clips_remix_host(x, m), fmt).tobytes(), w
        assert row[valid[w]:].tobytes() == np.full((T - valid[w], C_out), silence, dt).tobytes(), w
    assert owned.sum() == n
    assert (got[~owned].view(np.uint8) == 0xA5).all(), "a batch row outside the spans was written"
    # the same spans without dst_row: padded rows one after the other
    nb = n * T * C_out * dt.itemsize
    raw = call(be, clips, C_out, fmt, valid, None, off, np.full(misalign + nb + GUARD, 0xA5, np.uint8), misalign, n * T)
    assert raw[misalign:misalign + nb].tobytes() == got[dst // T].tobytes()
    assert (raw[:misalign] == 0xA5).all() and (raw[misalign + nb:] == 0xA5).all()


# ---------------------------------------------------------------------------------------------------------- 5. status codes
def test_status_codes(be):
    from frad_python_amd._lib import FradError
    z = be.put(np.zeros(64, np.int64))
    p = be.ptr(z)
    args = lambda C=2, code=22, n=1, rows=1, **nul: (
        nul.get("src_ptr", p), nul.get("src_ch", p), nul.get("mats", p), nul.get("mat_off", p), n, C, nul.get("valid", p), nul.get("dst_row", 0),
        code, 2, nul.get("out", p), nul.get("out_off", p), rows, be.stream)
    for bad in (dict(C=0), dict(C=-1), dict(code=16), dict(code=24), dict(code=-1), dict(n=-1), dict(rows=-1), dict(src_ptr=0), dict(src_ch=0),
                dict(mats=0), dict(mat_off=0), dict(valid=0), dict(out=0), dict(out_off=0)):
        with pytest.raises(FradError) as e:
            be.lib.clips_remix(*args(**bad))
        assert e.value.status == -1, bad                       # FRAD_E_INVALID
    nothing = dict(src_ptr=0, src_ch=0, mats=0, mat_off=0, valid=0, out=0, out_off=0)
    assert be.lib.clips_remix(*args(n=0, **nothing)) is None   # nothing to do: no table is read, nothing is launched
    assert be.lib.clips_remix(*args(rows=0, **nothing)) is None
    assert be.lib.clips_remix(*args()) is None                 # all-zero tables: one clip without rows, an empty span
    assert (be.get(z) == 0).all()


@pytest.mark.gpu
def test_core_wrapper_checks_everything_before_it_launches():
    """core.clips_remix: what the C-ABI cannot check (the tables live in device memory) is checked on the host."""
    import torch
    from frad_python_amd import core
    rng = np.random.default_rng(5)
    xs = [rng.uniform(-1, 1, (40, 2)), rng.uniform(-1, 1, (10, 1)), np.zeros((0, 3)), rng.uniform(-1, 1, (6, 3))]
    up = lambda a: torch.from_numpy(a).to("cuda:0")
    mats = {1: np.ones((2, 1)), 2: np.eye(2), 3: np.array([[1, 0, 0], [0, 0.5, 0.5]])}
    good = dict(srcs=[up(a) for a in xs], mats=mats, C_out=2, valid=None, fmt=None, span=None, dst_row=None, out=None)
    run = lambda kw: core.clips_remix(kw["srcs"], kw["mats"], kw["C_out"], kw["valid"], kw["fmt"], kw["span"], kw["dst_row"], kw["out"])
    out, off = run(good)
    want = np.concatenate([clips_remix_host(a, mats[a.shape[1]]) for a in xs])
    assert off.tolist() == [0, 40, 50, 50, 56] and np.array_equal(bits(out.cpu().numpy()), bits(want))
    per_clip = dict(good, mats=[mats[a.shape[1]] for a in xs], srcs=good["srcs"][:2] + [None] + good["srcs"][3:])
    assert np.array_equal(bits(run(per_clip)[0].cpu().numpy()), bits(want))
    s16 = run(dict(good, fmt="s16le"))[0].cpu().numpy()
    assert s16.reshape(-1)[:want.size * 2].tobytes() == from_f64(want, "s16le").tobytes()
    batch = torch.zeros((6, 40, 2), dtype=torch.float64, device="cuda:0")
    scatter = dict(good, span=[40] * 4, dst_row=[200, 0, 40, 120], out=batch)
    assert run(scatter)[0] is batch
    assert np.array_equal(batch[0, :10].cpu().numpy(), want[40:50]) and not batch[0, 10:].any() and not batch[1].any()
    assert np.array_equal(batch[5].cpu().numpy(), want[:40]) and np.array_equal(batch[3, :6].cpu().numpy(), want[50:])
    odd = torch.zeros(2 * 40 + 1, dtype=torch.float64, device="cuda:0")[1:].reshape(40, 2)[::2]
    for bad in (dict(C_out=0), dict(valid=[41, 10, 0, 6]), dict(valid=[40, 10, 0]), dict(valid=[40, -1, 0, 6]), dict(span=[39, 10, 0, 6]),
                dict(mats={1: mats[1], 2: mats[2]}), dict(mats={**mats, 3: np.ones((2, 2))}), dict(mats={**mats, 2: np.ones(2)}),
                dict(mats={**mats, 1: np.array([[np.inf], [1.0]])}), dict(mats={**mats, 2: np.full((2, 2), np.nan)}),
                dict(mats=[mats[2]]), dict(fmt="s17le"), dict(out=batch), dict(srcs=[odd] + good["srcs"][1:]),
                dict(srcs=[good["srcs"][0].float()] + good["srcs"][1:]), dict(srcs=[good["srcs"][0].reshape(-1)] + good["srcs"][1:]),
                dict(srcs=[None] + good["srcs"][1:], valid=[40, 10, 0, 6])):
        with pytest.raises(ValueError):
            run(dict(good, **bad))
            print("no ValueError for", [k for k in bad])
    with pytest.raises(RuntimeError):
        run(dict(good, srcs=[good["srcs"][0].cpu()] + good["srcs"][1:]))
    for bad in (dict(dst_row=[200, 0, 40, 39]), dict(dst_row=[201, 0, 40, 120]), dict(dst_row=[-1, 0, 40, 120]), dict(span=[39, 40, 40, 40]),
                dict(dst_row=[0, 40]), dict(out=None)):
        with pytest.raises(ValueError):
            run(dict(scatter, **bad))
            print("no ValueError for", [k for k in bad])
    with pytest.raises(TypeError):
        run(dict(scatter, out=batch.float()))


# ------------------------------------------------------------------------------------------------------------- 6. resources
def test_every_instantiation_is_built_without_scratch():
    """code-object metadata of the built library (tools/resources.py, no GPU needed)"""
    import sys
    from frad_python_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfrad_hip.so not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resources
    rows = {r["demangled"]: int(r.get("private_segment_fixed_size", 0)) for r in resources.kernels(_lib.LIB_PATH) if "k_clips_remix" in r["demangled"]}
    assert len(rows) == 11, sorted(rows)
    for name, scratch in rows.items():
        assert scratch == 0, f"{name}: {scratch} B of scratch per lane"
