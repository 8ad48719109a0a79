"""frad_clips_carry_cut alone: frad_clips_frame_cut for clips that are pieces of live streams -- every row is gathered from what
the stream carried over and the chunk that just arrived, and the remainder behind the last row is written for the next tick.

"emu": the CPU interpreter build of the same kernel source, "gpu": the MI355X.  Both legs call the C-ABI with raw pointers, so
that the guard bytes are the test's own: the carries lie in one buffer with 0x5A gaps, the remainders go into a buffer that is
0xA5 throughout, `out` sits between guards, and every byte that is not named must keep its fill.  The expected result is numpy
slicing of carry ++ chunk; a gather has no tolerance.  No data byte is zero and none is a fill byte's value by construction of
the check: the fills are compared where no data may be, the data where it must be."""
import numpy as np
import pytest

from test_clips_ola import be, Emu, Gpu, _backends  # noqa: F401  (the two backends and their fixture)

GUARD, GAP = 64, 32
SHIFTS = ((0, 0, 0), (1, 3, 7), (3, 7, 15), (7, 15, 1), (15, 1, 3))      # bytes off 16-byte alignment: out, src, carry / remainder slots


def virtual(clips):
    return [np.concatenate([c, s]) for c, s in clips]


def launch(be, clips, row_clip, row_at, row_len, step, next_at, shifts=(0, 0, 0), nxt="all"):
    """clips: [(carry bytes, chunk bytes)].  ``nxt``: "all", None (a NULL table) or the set of clips that get a remainder.
    -> (rows [n_rows, row_len * step], {clip: remainder bytes}); every guard, gap and unnamed slot is checked here."""
    out_shift, src_shift, slot_shift = shifts
    n, n_rows, rb = len(clips), len(row_clip), row_len * step
    V = virtual(clips)
    # the carries: one buffer, 0x5A between them
    c_at, pos = [], GAP
    for c, _ in clips:
        pos = (pos + 15) // 16 * 16 + slot_shift
        c_at.append(pos)
        pos += c.size + GAP
    carries = np.full(pos + GAP, 0x5A, np.uint8)
    for (c, _), a in zip(clips, c_at):
        carries[a:a + c.size] = c
    # the chunks, joined
    src_off = np.zeros(n + 1, np.int64)
    np.cumsum([s.size // step for _, s in clips], out=src_off[1:])
    joined = np.concatenate([s for _, s in clips]) if n else np.zeros(0, np.uint8)
    held = np.full(src_shift + joined.size + 16, 0x5A, np.uint8)
    held[src_shift:src_shift + joined.size] = joined
    # the remainders: 0xA5 throughout
    want = set(range(n)) if nxt == "all" else set(nxt or ())
    r_len = [V[j].size - int(next_at[j]) * step for j in range(n)]
    r_at, pos = [], GAP
    for j in range(n):
        pos = (pos + 15) // 16 * 16 + slot_shift
        r_at.append(pos)
        pos += r_len[j] + GAP
    rem = np.full(pos + GAP, 0xA5, np.uint8)
    d_car, d_src, d_rem = be.put(carries), be.put(held), be.put(rem)
    d_out = be.put(np.full(GUARD + out_shift + n_rows * rb + GUARD, 0xA5, np.uint8))
    i64 = lambda a: be.put(np.ascontiguousarray(a, np.int64) if len(a) else np.zeros(1, np.int64))
    i32 = lambda a: be.put(np.ascontiguousarray(a, np.int32) if len(a) else np.zeros(1, np.int32))
    d_cp = i64([be.ptr(d_car) + a if c.size else 0 for (c, _), a in zip(clips, c_at)])       # NULL where nothing is carried
    d_cl, d_so = i32([c.size // step for c, _ in clips]), i64(src_off)
    d_rc, d_ra, d_na = i32(row_clip), i64(row_at), i64(next_at)
    d_np = i64([be.ptr(d_rem) + r_at[j] if j in want else 0 for j in range(n)])
    be.lib.clips_carry_cut(be.ptr(d_cp), be.ptr(d_cl), be.ptr(d_src) + src_shift, be.ptr(d_so), n, be.ptr(d_rc), be.ptr(d_ra), n_rows,
                           row_len, step, be.ptr(d_out) + GUARD + out_shift, be.ptr(d_na), be.ptr(d_np) if nxt is not None else 0, be.stream)
    raw = be.get(d_out)
    lo = GUARD + out_shift
    assert (raw[:lo] == 0xA5).all() and (raw[lo + n_rows * rb:] == 0xA5).all(), "guard bytes around out were written"
    assert np.array_equal(be.get(d_car), carries) and np.array_equal(be.get(d_src), held), "a source was written"
    got_rem, mask, left = be.get(d_rem), np.ones(rem.size, bool), {}
    for j in sorted(want):
        left[j] = got_rem[r_at[j]:r_at[j] + r_len[j]].copy()
        mask[r_at[j]:r_at[j] + r_len[j]] = False
    assert (got_rem[mask] == 0xA5).all(), "bytes outside the named remainders were written"
    return raw[lo:lo + n_rows * rb].reshape(n_rows, rb), left


def expected_rows(clips, row_clip, row_at, row_len, step):
    V = virtual(clips)
    return np.stack([V[c][at * step:(at + row_len) * step] for c, at in zip(row_clip, row_at)]) if len(row_clip) else \
        np.zeros((0, row_len * step), np.uint8)


def check(be, clips, row_clip, row_at, row_len, step, next_at, shifts=(0, 0, 0), nxt="all"):
    V = virtual(clips)
    assert all(at >= 0 and (at + row_len) * step <= V[c].size for c, at in zip(row_clip, row_at))          # the test's own tables
    rows, left = launch(be, clips, row_clip, row_at, row_len, step, next_at, shifts, nxt)
    assert np.array_equal(rows, expected_rows(clips, row_clip, row_at, row_len, step)), (row_len, step, shifts)
    for j, got in left.items():
        assert np.array_equal(got, V[j][int(next_at[j]) * step:]), (j, row_len, step, shifts)


def data(rng, frames, step):
    return rng.integers(1, 256, frames * step, dtype=np.uint8)                       # no zero byte


def live_clips(rng, row_len, hop, step, total_rows=0):
    """A tick of the pool's shape: carries of 0, 1, row_len - hop and row_len - 1 sample-frames (those that differ) crossed with
    chunks that complete 0, 1, 2 and 7 rows -- a chunk of 0 and of 1 sample-frame among them -- shuffled; ``total_rows``: one more
    clip brings the launch to that many rows.  -> (clips, row_clip, row_at, next_at)"""
    shapes = []
    for ci, carry in enumerate(sorted({0, 1, row_len - hop, row_len - 1})):
        for k in (0, 1, 2, 7):
            if k == 0:
                room = row_len - 1 - carry                                           # have stays below one row
                chunk = (0, min(1, room), room, room // 2)[ci % 4]
            else:
                chunk = row_len + (k - 1) * hop + int(rng.integers(0, hop)) - carry  # exactly k rows
            shapes.append((carry, chunk))
    if total_rows:
        extra_rows = total_rows - 10 * len(shapes) // 4
        shapes.append((row_len - hop, row_len + (extra_rows - 1) * hop + hop // 2 - (row_len - hop)))
    shapes = [shapes[i] for i in rng.permutation(len(shapes))]
    clips = [(data(rng, c, step), data(rng, s, step)) for c, s in shapes]
    row_clip, row_at, next_at = [], [], []
    for j, (c, s) in enumerate(shapes):
        have = c + s
        k = (have - row_len) // hop + 1 if have >= row_len else 0
        row_clip += [j] * k
        row_at += [i * hop for i in range(k)]
        next_at.append(k * hop)
    return clips, row_clip, row_at, next_at


# step: 1 = u8 mono, 3 = s24 mono, 6 = three channels of s16 (no power of two), 16 = f64 stereo; row lengths whose byte size is
# (128) and is not (50, 3) a multiple of 16; hops that leave a carry of 0, half a row, and one sample-frame short of a row (the
# carry of row_len - hop = 1 sample-frame).  The tick's 40 rows, and enough rows for several blocks' tiles (16 KiB of output each)
@pytest.mark.parametrize("step", [1, 3, 6, 16])
@pytest.mark.parametrize("row_len", [128, 50, 3])
def test_rows_and_remainders_are_numpy_slices(be, step, row_len):
    rng = np.random.default_rng(step * 1000 + row_len)
    many = 40000 // (row_len * step) + 37
    for hop in sorted({row_len, row_len // 2, row_len - 1} - {0}):
        for total in (0, many):
            clips, rc, ra, na = live_clips(rng, row_len, hop, step, total)
            assert len(rc) == (total or 10 * (len(clips) // 4))
            for shifts in SHIFTS if total else SHIFTS[:1] + SHIFTS[2:3]:
                check(be, clips, rc, ra, row_len, step, na, shifts)


@pytest.mark.parametrize("step", [1, 3, 6, 16])
def test_one_row(be, step):
    rng = np.random.default_rng(step)
    for row_len in (128, 50, 3):
        for carry in (0, 1, row_len - 1, row_len):
            clips = [(data(rng, carry, step), data(rng, row_len - carry + 2, step))]
            for shifts in SHIFTS:
                check(be, clips, [0], [1 if carry != row_len else 0], row_len, step, [row_len], shifts)


def test_rows_in_the_carry_in_the_chunk_and_across_the_seam(be):
    """row_len 50, a carry of 70 sample-frames, `out` aligned.  Row 0 (at 0) lies wholly in the carry, row 1 (at 70) wholly in the
    chunk, the others across the seam.  At step 1 row 3 begins at output byte 150 and its seam (at 64: 6 bytes in) is byte 156,
    inside the 16-byte store [144, 160); row 4 begins at byte 200 and its seam (at 62: 8 bytes in) is byte 208 = 13 * 16, a store
    boundary.  Rows at 69 and 21 keep one sample-frame on one side of the seam."""
    rng = np.random.default_rng(11)
    for step, carry in ((1, 70), (6, 70), (16, 70)):
        clips = [(data(rng, carry, step), data(rng, 300, step))]
        ra = [0, 70, 38, 64, 62, 20, 69, 21]
        check(be, clips, [0] * len(ra), ra, 50, step, [5])
        check(be, clips, [0] * len(ra), ra, 50, step, [5], (0, 1, 0))


def test_next_at_in_the_carry_at_the_seam_in_the_chunk_and_at_the_end(be):
    rng = np.random.default_rng(12)
    for step in (1, 3, 16):
        carry, chunk = 40, 90
        clips = [(data(rng, carry, step), data(rng, chunk, step)) for _ in range(7)] + [(data(rng, 0, step), data(rng, 0, step))]
        next_at = [0, 17, 40, 41, 129, 130, 39, 0]               # all of V; in the carry; the seam; in the chunk; one left; none; ...
        rc, ra = [0, 3, 3, 6], [0, 80, 30, 10]
        for shifts in SHIFTS:
            check(be, clips, rc, ra, 50, step, next_at, shifts)
        check(be, clips, rc, ra, 50, step, next_at, nxt={0, 2, 5, 6})               # NULL per clip: those clips write nothing
        check(be, clips, rc, ra, 50, step, next_at, nxt=None)                       # NULL as a table
        check(be, clips, [], [], 50, step, next_at)                                 # no row at all: the remainders alone
        check(be, clips, [], [], 50, step, next_at, nxt=None)                       # ... and nothing to do


@pytest.mark.parametrize("step,row_len,hop", [(6, 50, 25), (1, 128, 127), (3, 3, 1), (16, 50, 50)])
def test_a_chain_of_launches_is_one_cut_of_the_whole_sequence(be, step, row_len, hop):
    """Three streams, each a byte sequence cut into seeded random chunks (empty ones among them), fed through successive launches:
    the remainders a launch wrote are the next launch's carries.  All rows together are frad_clips_frame_cut of the same build
    over the whole sequence, and numpy's."""
    rng = np.random.default_rng(step * 100 + hop)
    total = [row_len + 23 * hop + 7, 3 * row_len + 5, row_len - 1 + 40 * hop]
    seqs = [data(rng, t, step) for t in total]
    fed, carry, rows_of = [0] * 3, [np.zeros(0, np.uint8) for _ in range(3)], [[] for _ in range(3)]
    launches = 0
    while any(f < t for f, t in zip(fed, total)):
        clips, rc, ra, na = [], [], [], []
        for j in range(3):
            n = min(int(rng.choice([0, 0, 1, hop // 2, hop, row_len, 2 * row_len + 3, int(rng.integers(0, 4 * row_len))])), total[j] - fed[j])
            clips.append((carry[j], seqs[j][fed[j] * step:(fed[j] + n) * step]))
            fed[j] += n
            have = carry[j].size // step + n
            k = (have - row_len) // hop + 1 if have >= row_len else 0
            rc += [j] * k
            ra += [i * hop for i in range(k)]
            na.append(k * hop)
        rows, left = launch(be, clips, rc, ra, row_len, step, na, SHIFTS[launches % 5])
        for r, j in enumerate(rc):
            rows_of[j].append(rows[r])
        carry = [left[j] for j in range(3)]
        launches += 1
    assert launches > 5
    for j in range(3):
        k = (total[j] - row_len) // hop + 1
        src = np.arange(k, dtype=np.int64) * hop
        want = np.stack([seqs[j][a * step:(a + row_len) * step] for a in src])
        assert np.array_equal(np.stack(rows_of[j]), want), j
        assert np.array_equal(carry[j], seqs[j][k * hop * step:]), j
        d_src, d_rs, d_rv = be.put(seqs[j]), be.put(src), be.put(np.full(k, row_len, np.int32))
        d_out = be.put(np.zeros(k * row_len * step, np.uint8))
        be.lib.clips_frame_cut(be.ptr(d_src), be.ptr(d_rs), be.ptr(d_rv), k, row_len, step, be.ptr(d_out), be.stream)
        assert np.array_equal(be.get(d_out).reshape(k, -1), np.stack(rows_of[j])), j


def test_invalid_arguments_are_refused_and_nothing_is_written(be):
    from frad_python_amd._lib import FradError
    z = be.put(np.zeros(64, np.int64))
    out, rem = be.put(np.full(256, 0xA5, np.uint8)), be.put(np.full(256, 0xA5, np.uint8))
    ptrs = be.put(np.array([be.ptr(rem)] + [0] * 7, np.int64))
    p = be.ptr

    def args(**kw):
        a = dict(carry_ptr=p(z), carry_len=p(z), src=p(z), src_off=p(z), n_clips=1, row_clip=p(z), row_at=p(z), n_rows=1, row_len=4,
                 step=4, out=p(out), next_at=p(z), next_ptr=p(ptrs))
        a.update(kw)
        return list(a.values()) + [be.stream]

    for bad in (dict(step=0), dict(step=-1), dict(row_len=0), dict(row_len=-5), dict(n_clips=-1), dict(n_rows=-1), dict(carry_ptr=0),
                dict(carry_len=0), dict(src=0), dict(src_off=0), dict(row_clip=0), dict(row_at=0), dict(out=0), dict(next_at=0)):
        with pytest.raises(FradError) as e:
            be.lib.clips_carry_cut(*args(**bad))
        assert e.value.status == -1, bad
    assert be.lib.clips_carry_cut(*args(n_clips=0)) is None                          # no clip: nothing is looked at
    assert be.lib.clips_carry_cut(*args(n_clips=0, carry_ptr=0, src=0, out=0)) is None
    assert be.lib.clips_carry_cut(*args(n_rows=0, next_ptr=0, out=0, row_clip=0, row_at=0)) is None        # nothing to write
    assert (be.get(out) == 0xA5).all() and (be.get(rem) == 0xA5).all()


def test_core_wrapper_checks_the_tables_before_it_launches():
    """core.clips_carry_cut: what the C-ABI cannot check (the tables live in device memory) is checked on the host, before
    anything is uploaded -- so host tensors get that far, and the tables are refused before the tensors are."""
    import torch
    from frad_python_amd import core
    step, row_len = 6, 50
    src = torch.from_numpy(np.random.default_rng(1).integers(1, 256, 200 * step + 4, dtype=np.uint8))       # 200 sample-frames, 4 stray bytes
    carry = [torch.ones(30 * step, dtype=torch.uint8), None]
    ok = dict(carry=carry, src=src, so=[0, 120, 200], rc=[0, 0, 1], ra=[0, 100, 30], row_len=row_len, step=step, na=[150, 80],
              nxt=[torch.zeros(0, dtype=torch.uint8), torch.zeros(0, dtype=torch.uint8)])
    run = lambda kw: core.clips_carry_cut(kw["carry"], kw["src"], kw["so"], kw["rc"], kw["ra"], kw["row_len"], kw["step"], kw["na"], kw["nxt"])
    with pytest.raises(ValueError, match="device memory"):                            # the tables pass; the host tensors do not
        run(ok)
    for bad, why in ((dict(ra=[0, 101, 30]), "end inside"), (dict(ra=[0, 100, 31]), "end inside"), (dict(ra=[-1, 100, 30]), "end inside"),
                     (dict(ra=[(1 << 63) - 50, 0, 0]), "end inside"), (dict(rc=[0, 2, 1]), "not there"), (dict(rc=[0, -1, 1]), "not there"),
                     (dict(rc=[0, 0]), "one entry per row"), (dict(na=[151, 80]), "next_at"), (dict(na=[150, -1]), "next_at"),
                     (dict(na=[150]), "one entry per clip"), (dict(nxt=[None]), "one entry per clip"), (dict(so=[0, 120, 201]), "inside src"),
                     (dict(so=[0, 120, 100]), "not decrease"), (dict(so=[-1, 120, 200]), "not decrease"), (dict(so=[0, 120]), "one per clip"),
                     (dict(carry=[torch.ones(31, dtype=torch.uint8), None]), "whole sample-frames"),
                     (dict(carry=[torch.ones(30, dtype=torch.int16), None]), "whole sample-frames"), (dict(src=src.view(torch.int16)), "1-D uint8"),
                     (dict(row_len=0), "geometry"), (dict(step=0), "geometry"),
                     (dict(nxt=[torch.zeros(step, dtype=torch.uint8), None]), r"nxt\[0\]")):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match=why):
            run(kw)


@pytest.mark.gpu
def test_bridge_method_equals_the_numpy_model():
    import torch
    from frad_python_amd.bridge import HipBridge
    from frad_python_amd.pool import clips_carry_cut_host
    br, rng, step, row_len, hop = HipBridge(), np.random.default_rng(3), 6, 50, 25
    clips, rc, ra, na = live_clips(rng, row_len, hop, step, 340)
    up = lambda a: torch.from_numpy(a).to(br.device)
    carry = [None if not c.size else c for c, _ in clips]
    src_off = np.zeros(len(clips) + 1, np.int64)
    np.cumsum([s.size // step for _, s in clips], out=src_off[1:])
    src = np.concatenate([s for _, s in clips])
    want, want_next = clips_carry_cut_host(carry, src, src_off, rc, ra, row_len, step, na)
    dev_carry = [None if c is None else up(c) for c in carry]
    rows, nxt = br.clips_carry_cut(dev_carry, up(src), src_off, rc, ra, row_len, step, na)
    assert np.array_equal(rows.cpu().numpy(), want) and np.array_equal(want, expected_rows(clips, rc, ra, row_len, step))
    for j in range(len(clips)):
        assert np.array_equal(nxt[j].cpu().numpy(), want_next[j]), j
        assert dev_carry[j] is None or np.array_equal(dev_carry[j].cpu().numpy(), carry[j])
    with pytest.raises(ValueError, match="overlaps"):                                 # a remainder over a carry is refused
        br.core.clips_carry_cut(dev_carry, up(src), src_off, rc, ra, row_len, step, na,
                                [dev_carry[j][:nxt[j].numel()] if dev_carry[j] is not None and 0 < nxt[j].numel() <= dev_carry[j].numel()
                                 else nxt[j] for j in range(len(clips))])
