"""Reed-Solomon protection and repair (csrc/frad_ecc.hip: frad_rs_encode / frad_rs_repair) against a host model of the
code the reference uses (tools/ecc.py: reedsolo.RSCodec(codesize, dsize + codesize), GF(2^8) over 0x11d, alpha = 2, first
consecutive root 0).  The model below is written from that definition; the decoder is checked as a bounded-distance
decoder: within t = codesize // 2 errors the unique codeword, beyond it either zeros or exactly the data of a codeword
within t.  "emu": the same kernel source under the CPU interpreter (tests/emu); "gpu": the MI355X."""
import functools

import numpy as np
import pytest

from frad_python_amd import ecc

# ---------------------------------------------------------------------------------------------------------- host model
EXP = np.zeros(512, np.int64)
LOG = np.zeros(256, np.int64)
_x = 1
for _i in range(255):
    EXP[_i] = EXP[_i + 255] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D
MUL = np.zeros((256, 256), np.uint8)
MUL[1:, 1:] = EXP[(LOG[1:, None] + LOG[None, 1:])]


@functools.lru_cache(maxsize=None)
def gen_poly(cs):
    """coefficients of prod_{i < cs} (x - alpha^i), highest power first"""
    g = [1]
    for i in range(cs):
        a = int(EXP[i])
        g = [(g[j] if j < len(g) else 0) ^ (int(MUL[g[j - 1], a]) if j >= 1 else 0) for j in range(len(g) + 1)]
    return np.array(g, np.uint8)


def parity(blocks: np.ndarray, cs: int) -> np.ndarray:
    """check bytes of every row of `blocks` [nb, k] (remainder of data * x^cs by g), vectorised over the rows"""
    nb, k = blocks.shape
    r = np.zeros((nb, cs), np.uint8)
    if cs == 0:
        return r
    g = gen_poly(cs)[1:]                                      # g_(cs-1) .. g_0 (monic term dropped)
    for j in range(k):
        fb = blocks[:, j] ^ r[:, 0]
        r[:, :-1] = r[:, 1:]
        r[:, -1] = 0
        r ^= MUL[fb[:, None], g[None, :]]
    return r


def model_encode(data: bytes, dsize: int, cs: int) -> bytes:
    """ecc.encode (tools/ecc.py:6-12): every dsize-byte chunk followed by its check bytes, the last chunk shortened"""
    full = len(data) // dsize
    body = np.frombuffer(data[:full * dsize], np.uint8).reshape(full, dsize)
    out = np.concatenate([body, parity(body, cs)], 1).tobytes()
    if len(data) % dsize:
        tail = np.frombuffer(data[full * dsize:], np.uint8)[None, :]
        out += tail.tobytes() + parity(tail, cs).tobytes()
    return out


def syndromes(block: np.ndarray, cs: int) -> np.ndarray:
    s = np.zeros(cs, np.int64)
    for i in range(cs):
        v = 0
        for b in block:
            v = (int(EXP[LOG[v] + i]) if v else 0) ^ int(b)
        s[i] = v
    return s


def blocks_of(data: bytes, size: int):
    return [np.frombuffer(data[i:i + size], np.uint8) for i in range(0, len(data), size)]


# ------------------------------------------------------------------------------------------------------------ backends
class EmuEcc:
    """frad_rs_encode / frad_rs_repair of the CPU interpreter build, with numpy buffers (the bridge interface)."""

    def __init__(self):
        from helpers import build_emulator
        from frad_python_amd._lib import FradLib
        self.lib = FradLib(build_emulator())
        self.scan_lib = self.lib

    def _run(self, payloads, dsize, cs, repair):
        buf, head, n_blocks, out_off = ecc.pack(payloads, dsize, cs, repair)
        n1 = len(payloads) + 1
        p = buf.ctypes.data
        nout = int(out_off[-1])
        out = np.zeros(nout + 32, np.uint8)
        return buf, (p, p + head, p + head + 8 * n1, p + head + 16 * n1), n_blocks, out_off, out

    def rs_encode(self, payloads, dsize, cs, crc32=False):
        import zlib
        if not payloads:
            return ([], []) if crc32 else []
        buf, ptrs, nb, off, out = self._run(payloads, dsize, cs, False)
        self.lib.rs_encode(*ptrs, len(payloads), nb, dsize, cs, out.ctypes.data)
        outs = [out[off[i]:off[i + 1]].tobytes() for i in range(len(payloads))]
        return (outs, [zlib.crc32(o) for o in outs]) if crc32 else outs

    def rs_repair(self, payloads, dsize, cs):
        n = len(payloads)
        if n == 0:
            return [], np.zeros(0, np.int32), np.zeros(0, np.int32)
        buf, ptrs, nb, off, out = self._run(payloads, dsize, cs, True)
        cnt = np.zeros(2 * n + nb + 1, np.int32)
        c = cnt.ctypes.data
        self.lib.rs_repair(*ptrs, n, nb, dsize, cs, out.ctypes.data, c, c + 4 * n, c + 8 * n)
        return [out[off[i]:off[i + 1]].tobytes() for i in range(n)], cnt[:n].copy(), cnt[n:2 * n].copy()


def make_backend(kind):
    if kind == "emu":
        return EmuEcc()
    from frad_python_amd.bridge import HipBridge
    return HipBridge()


@pytest.fixture(params=[pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)], scope="module")
def bk(request):
    return make_backend(request.param)


# --------------------------------------------------------------------------------------------------------- known answer
HELLO = b"hello world\xed%T\xc4\xfd\xfd\x89\xf3\xa8\xaa"            # reedsolo's README: RSCodec(10).encode(b'hello world')


def test_known_answer_model():
    assert model_encode(b"hello world", 245, 10) == HELLO
    assert not syndromes(np.frombuffer(HELLO, np.uint8), 10).any()


def test_known_answer_kernels(bk):
    assert bk.rs_encode([b"hello world"], 245, 10) == [HELLO]
    assert bk.rs_encode([], 245, 10) == [] and bk.rs_encode([], 245, 10, crc32=True) == ([], [])    # no payloads: nothing launched
    damaged = bytearray(HELLO)
    damaged[0] ^= 0x55; damaged[7] ^= 1; damaged[-1] ^= 0xFF
    fixed, cor, bad = bk.rs_repair([bytes(damaged), HELLO], 245, 10)
    assert fixed == [b"hello world", b"hello world"] and cor.tolist() == [1, 0] and bad.tolist() == [0, 0]


# -------------------------------------------------------------------------------------------------------------- encode
RATIOS = [(96, 24), (223, 32), (1, 254), (254, 1), (17, 0), (5, 3)]


def _lengths(dsize, big):
    ls = [0, 1, max(dsize - 1, 1), 3 * dsize, 3 * dsize + max(dsize // 3, 1)]
    return ls + ([70001] if big else [])


@pytest.mark.parametrize("ratio", RATIOS)
def test_encode_matches_model(bk, ratio):
    dsize, cs = ratio
    rng = np.random.default_rng(dsize * 1000 + cs)
    big = isinstance(bk, EmuEcc) is False or ratio in ((96, 24), (5, 3))
    lens = _lengths(dsize, big) * 3
    payloads = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    got = bk.rs_encode(payloads, dsize, cs)
    for p, g in zip(payloads, got):
        assert g == model_encode(p, dsize, cs)
        for blk in blocks_of(g, dsize + cs)[:3] + blocks_of(g, dsize + cs)[-1:]:
            assert not syndromes(blk, cs).any()


def test_encode_validates_ratio(bk):
    from frad_python_amd._lib import FradError
    for bad in ((0, 10), (200, 56), (-1, 3)):
        with pytest.raises((FradError, ValueError)):     # the host plan or the C-ABI refuses it
            bk.rs_encode([b"abc"], *bad)


# -------------------------------------------------------------------------------------------------------------- repair
def _damage(rng, block: bytearray, e: int, must=()):
    pos = list(must) + [int(p) for p in rng.permutation(len(block)) if p not in must]
    for p in pos[:e]:
        block[p] ^= int(rng.integers(1, 256))


@pytest.mark.parametrize("ratio", [(96, 24), (223, 32), (5, 3), (1, 254), (17, 0)])
def test_repair_within_t_is_exact(bk, ratio):
    dsize, cs = ratio
    t = cs // 2
    rng = np.random.default_rng(7 + cs)
    n_frames = 6 if cs < 200 else 3
    payloads = [rng.integers(0, 256, int(rng.integers(1, 6 * dsize + 2)), dtype=np.uint8).tobytes() for _ in range(n_frames)]
    payloads.append(rng.integers(0, 256, 2 * dsize + 1, dtype=np.uint8).tobytes())     # a shortened last block
    prot = [model_encode(p, dsize, cs) for p in payloads]
    damaged, want_cor = [], []
    for f, q in enumerate(prot):
        blocks = [bytearray(b.tobytes()) for b in blocks_of(q, dsize + cs)]
        cor = 0
        for i, blk in enumerate(blocks):
            e = int(rng.integers(0, t + 1)) if i % 3 else t        # every third block carries the full t errors
            must = (len(blk) - 1, len(blk) - 1 - cs) if len(blk) > cs else ()   # a check byte and the block's last data byte
            _damage(rng, blk, e, must[:e])
            cor += e > 0 and len(blk) > cs
        damaged.append(b"".join(bytes(b) for b in blocks))
        want_cor.append(cor)
    fixed, cor, bad = bk.rs_repair(damaged, dsize, cs)
    assert fixed == payloads
    assert bad.tolist() == [0] * len(payloads)
    assert cor.tolist() == (want_cor if cs else [0] * len(payloads))
    # undamaged input comes back unchanged, nothing counted
    fixed, cor, bad = bk.rs_repair(prot, dsize, cs)
    assert fixed == payloads and not cor.any() and not bad.any()


def test_repair_beyond_t_brute_force(bk):
    """(2, 4) and its shortened (1, 4) blocks: the whole codebook is small enough to search"""
    dsize, cs, t = 2, 4, 2
    rng = np.random.default_rng(11)
    books = {}
    for k in (1, 2):
        data = np.array(np.meshgrid(*[np.arange(256)] * k, indexing="ij")).reshape(k, -1).T.astype(np.uint8)
        books[k] = (data, np.concatenate([data, parity(data, cs)], 1))
    frames, want, want_bad = [], [], []
    for i in range(300):
        k = 2 if i % 3 else 1
        data = rng.integers(0, 256, k, dtype=np.uint8)
        blk = bytearray(data.tobytes() + parity(data[None, :], cs).tobytes())
        _damage(rng, blk, int(rng.integers(t + 1, cs + k + 1)))
        d, cw = books[k]
        dist = (cw != np.frombuffer(bytes(blk), np.uint8)[None, :]).sum(1)
        near = np.nonzero(dist <= t)[0]
        assert near.size <= 1
        frames.append(bytes(blk))
        want.append(d[near[0]].tobytes() if near.size else bytes(k))
        want_bad.append(0 if near.size else 1)
    fixed, cor, bad = bk.rs_repair(frames, dsize, cs)
    assert fixed == want
    assert bad.tolist() == want_bad and (cor + bad).tolist() == [1] * len(frames)


def test_repair_beyond_t_large_code(bk):
    """(96, 24) with t + 1 .. 24 errors: zeros (counted as failed) or exactly a codeword within t of what was stored"""
    dsize, cs, t = 96, 24, 12
    rng = np.random.default_rng(5)
    frames = []
    for i in range(40):
        data = rng.integers(0, 256, dsize, dtype=np.uint8)
        blk = bytearray(data.tobytes() + parity(data[None, :], cs).tobytes())
        _damage(rng, blk, int(rng.integers(t + 1, cs + 1)))
        frames.append(bytes(blk))
    fixed, cor, bad = bk.rs_repair(frames, dsize, cs)
    for f, out, c, b in zip(frames, fixed, cor, bad):
        if b:
            assert out == bytes(dsize) and c == 0
        else:
            cw = np.frombuffer(model_encode(out, dsize, cs), np.uint8)
            assert (cw != np.frombuffer(f, np.uint8)).sum() <= t and c == 1


def test_repair_short_tail_and_codesize_zero(bk):
    # a trailing block no longer than codesize has an empty data part (the reference's negative slice)
    prot = model_encode(b"x" * 10, 5, 3)[:-0 or None] + b"\x01\x02"
    assert bk.rs_repair([prot], 5, 3)[0] == [b"x" * 10]
    assert ecc.data_len(len(prot), 5, 3) == 10
    # codesize 0: nothing to correct, the data passes through
    fixed, cor, bad = bk.rs_repair([b"abcdef" * 7, b""], 17, 0)
    assert fixed == [b"abcdef" * 7, b""] and not cor.any() and not bad.any()


def test_plan_matches_the_reference_slicing():
    from frad_python_amd.frames import strip_ecc
    rng = np.random.default_rng(1)
    for dsize, cs in RATIOS + [(0, 5), (3, 250)]:
        for n in (0, 1, 2, cs, cs + 1, dsize + cs, 3 * (dsize + cs) + 1, 1000):
            assert ecc.data_len(n, dsize, cs) == len(strip_ecc(rng.bytes(n), dsize, cs))
