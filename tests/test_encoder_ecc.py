"""Reed-Solomon-protected streams written by the Encoder (``Encoder(..., allow_ecc=True)`` + ``set_ecc(True, ratio)``, the
reference's encoder.py:102 and :201-209) and the two kernels behind them: frad_rs_encode_frames (fixed-stride ecc.encode of
equal-length payloads) and frad_crc16_ansi_frames (the compact ECC header's checksum of ragged frames).

Byte contract: the protected stream equals Repairer(r).process(plain) + flush() of the same encoder's stream without ECC,
and it equals an independent expectation: the unprotected payloads, the host GF(2^8) model below, then ASFH.write.
"emu": oracle arithmetic for the transform and the CPU interpreter of the HIP kernels; "gpu": the MI355X."""
import functools

import numpy as np
import pytest

from frad_python_amd import Decoder, Encoder, Repairer, core, synth
from frad_python_amd.common import crc16_ansi
from frad_python_amd.fourier import profiles
from frad_python_amd.tools.asfh import ASFH

# ---------------------------------------------------------------------------------------------------------- host model
# GF(2^8) over 0x11d, alpha = 2, generator prod_{i < cs} (x - alpha^i), systematic: the code of reedsolo.RSCodec that the
# reference's tools/ecc.py uses
_EXP = np.zeros(512, np.int64)
_LOG = np.zeros(256, np.int64)
_v = 1
for _i in range(255):
    _EXP[_i] = _EXP[_i + 255] = _v
    _LOG[_v] = _i
    _v <<= 1
    if _v & 0x100:
        _v ^= 0x11D
GF_MUL = np.zeros((256, 256), np.uint8)
GF_MUL[1:, 1:] = _EXP[_LOG[1:, None] + _LOG[None, 1:]]


@functools.lru_cache(maxsize=None)
def generator(cs):
    """g_(cs-1) .. g_0 of the monic generator polynomial (highest power first, the leading 1 dropped)"""
    g = [1]
    for i in range(cs):
        a = int(_EXP[i])
        nxt = g + [0]
        for j in range(1, len(g) + 1):
            nxt[j] ^= int(GF_MUL[g[j - 1], a])
        g = nxt
    return np.array(g[1:], np.uint8)


def check_bytes(rows: np.ndarray, cs: int) -> np.ndarray:
    """remainder of every row [n, k] times x^cs by g, vectorised over rows"""
    r = np.zeros((rows.shape[0], cs), np.uint8)
    if cs == 0:
        return r
    g = generator(cs)
    for j in range(rows.shape[1]):
        fb = rows[:, j] ^ r[:, 0]
        r[:, :-1] = r[:, 1:]
        r[:, -1] = 0
        r ^= GF_MUL[fb[:, None], g[None, :]]
    return r


def rs_model(data: bytes, dsize: int, cs: int) -> bytes:
    """ecc.encode: every dsize-byte chunk followed by its check bytes, the last chunk shortened"""
    full = len(data) // dsize
    body = np.frombuffer(data[:full * dsize], np.uint8).reshape(full, dsize)
    out = np.concatenate([body, check_bytes(body, cs)], 1).tobytes()
    if len(data) % dsize:
        tail = np.frombuffer(data[full * dsize:], np.uint8)[None, :]
        out += tail.tobytes() + check_bytes(tail, cs).tobytes()
    return out


def test_model_known_answer():
    # reedsolo's README: RSCodec(10).encode(b'hello world')
    assert rs_model(b"hello world", 245, 10) == b"hello world\xed%T\xc4\xfd\xfd\x89\xf3\xa8\xaa"


# ------------------------------------------------------------------------------------------------------------ backends
class EmuEncoderBridge:
    """The Encoder's / Decoder's / Repairer's bridge on the CPU: the oracle for the transform (helpers.OracleBridge,
    tests/test_p2_encode.py for profile 2), the interpreted HIP build for Reed-Solomon, the checksums and the header scan.
    ``lossless_encode_stream`` and ``rs_encode_crc16`` are the HipBridge methods of this feature, with numpy buffers."""

    def __init__(self):
        from helpers import OracleBridge
        from test_ecc import EmuEcc
        from test_p2_encode import EmuP2Enc
        self.inner, self.p2 = OracleBridge(), EmuP2Enc()
        self.rs = EmuEcc()
        self.lib = self.scan_lib = self.rs.lib
        self.rs_encode, self.rs_repair = self.rs.rs_encode, self.rs.rs_repair

    def __getattr__(self, name):
        if name.startswith("p2_"):
            return getattr(self.p2, name)
        return getattr(self.inner, name)

    # kernels with numpy buffers
    def rs_encode_frames(self, rows: np.ndarray, nbytes, dsize, cs, out: np.ndarray, out_offset=0):
        self.lib.rs_encode_frames(rows.ctypes.data, rows.strides[0], rows.shape[0], nbytes, dsize, cs,
                                  out.ctypes.data + out_offset, out.strides[0])

    def crc16_frames(self, data: bytes, offsets: np.ndarray) -> list:
        buf = np.frombuffer(data + bytes(16), np.uint8).copy()
        off = np.ascontiguousarray(offsets, np.int64)
        out = np.zeros(max(len(off) - 1, 1), np.uint16)
        self.lib.crc16_ansi_frames(buf.ctypes.data, off.ctypes.data, len(off) - 1, out.ctypes.data)
        return out[:len(off) - 1].tolist()

    # the HipBridge interface
    def lossless_encode_stream(self, profile, pcm, fmt, n_frames, N, C, bits, little_endian, head_fn, raw_be_ints=True,
                               ecc_ratio=None):
        frames = self.inner.lossless_encode(profile, pcm, fmt, n_frames, N, C, bits, little_endian, raw_be_ints)
        if any(b != frames[0][1] for _, b in frames) or frames[0][1] != (bits if bits in core.DEPTHS else 16):
            return None
        nb = len(frames[0][0])
        rows = np.zeros((n_frames, nb + 5), np.uint8)                    # an odd row stride: unaligned reads
        for i, (p, _) in enumerate(frames):
            rows[i, :nb] = np.frombuffer(p, np.uint8)
        plen = nb if ecc_ratio is None else core.rs_protected_bytes(nb, *ecc_ratio)
        stream = np.zeros((n_frames, 32 + plen), np.uint8)
        if ecc_ratio is None:
            stream[:, 32:] = rows[:, :nb]
        else:
            self.rs_encode_frames(rows, nb, *ecc_ratio, stream, 32)
        crc = np.zeros(n_frames, np.uint32)
        self.lib.crc32_frames(stream.ctypes.data + 32, stream.strides[0], n_frames, plen, crc.ctypes.data)
        stream[:, :28] = np.frombuffer(head_fn(plen), np.uint8)
        stream[:, 28:32] = crc.astype(">u4").view(np.uint8).reshape(n_frames, 4)
        return stream.tobytes()

    def rs_encode_crc16(self, payloads, dsize, cs):
        prot = self.rs.rs_encode(payloads, dsize, cs)
        off = np.zeros(len(prot) + 1, np.int64)
        np.cumsum([len(p) for p in prot], out=off[1:])
        return prot, self.crc16_frames(b"".join(prot), off)


class GpuKernels:
    """The two kernels through core on the MI355X, with numpy buffers in and out."""

    def __init__(self):
        import torch
        from frad_python_amd.bridge import HipBridge
        self.t, self.bridge = torch, HipBridge()
        self.dev = self.bridge.device

    def rs_encode_frames(self, rows: np.ndarray, nbytes, dsize, cs, out: np.ndarray, out_offset=0):
        t = self.t
        d_in = t.from_numpy(rows).to(self.dev)
        d_out = t.from_numpy(out).to(self.dev)
        core.rs_encode_frames(d_in, nbytes, dsize, cs, out=d_out[:, out_offset:])
        out[...] = d_out.cpu().numpy()

    def crc16_frames(self, data: bytes, offsets: np.ndarray) -> list:
        t = self.t
        d = t.from_numpy(np.frombuffer(data + bytes(1), np.uint8).copy()).to(self.dev)
        o = t.from_numpy(np.ascontiguousarray(offsets, np.int64)).to(self.dev)
        return core.crc16_ansi_frames(d, o).cpu().numpy().view(np.uint16).tolist()


@pytest.fixture(params=[pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)], scope="module")
def kind(request):
    return request.param


@pytest.fixture(scope="module")
def br(kind):
    if kind == "emu":
        return EmuEncoderBridge()
    from frad_python_amd.bridge import HipBridge
    return HipBridge()


@pytest.fixture(scope="module")
def kern(kind, br):
    return br if kind == "emu" else GpuKernels()


# ------------------------------------------------------------------------------------------------ kernel vs host model
RATIOS = [(96, 24), (223, 32), (1, 254), (255, 0), (16, 16)]


def _sizes(dsize):
    return sorted({max(dsize - 1, 1), dsize, 3 * dsize, 3 * dsize + 1, 70 * dsize + 1})


@pytest.mark.parametrize("ratio", RATIOS)
def test_rs_encode_frames_matches_model(kern, kind, ratio):
    dsize, cs = ratio
    rng = np.random.default_rng(dsize * 7 + cs)
    for nbytes in _sizes(dsize):
        for n in ((1, 3) if kind == "emu" else (1, 3, 67)):
            P = core.rs_protected_bytes(nbytes, dsize, cs)
            rows = rng.integers(0, 256, (n, nbytes + 3), dtype=np.uint8)
            out = np.full((n, 32 + P + 11), 0xA5, np.uint8)              # header hole and a tail gap that must stay untouched
            kern.rs_encode_frames(rows, nbytes, dsize, cs, out, 32)
            for f in range(n):
                assert out[f, 32:32 + P].tobytes() == rs_model(rows[f, :nbytes].tobytes(), dsize, cs), (nbytes, n, f)
            assert (out[:, :32] == 0xA5).all() and (out[:, 32 + P:] == 0xA5).all()


def test_rs_encode_frames_matches_the_ragged_kernel(br, kern):
    rng = np.random.default_rng(3)
    for dsize, cs in ((96, 24), (5, 3)):
        rows = rng.integers(0, 256, (4, 1000), dtype=np.uint8)
        P = core.rs_protected_bytes(1000, dsize, cs)
        out = np.zeros((4, P), np.uint8)
        kern.rs_encode_frames(rows, 1000, dsize, cs, out)
        assert [r.tobytes() for r in out] == br.rs_encode([r.tobytes() for r in rows], dsize, cs)


def test_rs_encode_frames_validates(kind):
    if kind == "emu":
        pytest.skip("core validates device tensors")
    import torch
    x = torch.zeros((2, 100), dtype=torch.uint8, device="cuda")
    for bad in ((0, 10), (200, 56), (10, -1)):
        with pytest.raises(ValueError):
            core.rs_encode_frames(x, 100, *bad)
    with pytest.raises(ValueError):
        core.rs_encode_frames(x, 101, 96, 24)                            # rows shorter than nbytes
    with pytest.raises(ValueError):
        core.rs_encode_frames(x, 100, 96, 24, out=torch.zeros((2, 120), dtype=torch.uint8, device="cuda"))   # P = 148
    with pytest.raises(RuntimeError):
        core.rs_encode_frames(x.cpu(), 100, 96, 24)
    with pytest.raises(ValueError):
        core.crc16_ansi_frames(torch.zeros(10, dtype=torch.uint8, device="cuda"), torch.tensor([0, 11], device="cuda"))


def test_crc16_frames_match_the_host(kern):
    rng = np.random.default_rng(9)
    lens = [0, 1, 2, 15, 16, 17, 255, 4096, 70000, 3]
    data = rng.integers(0, 256, sum(lens) + 7, dtype=np.uint8).tobytes()
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    off += 7                                                             # ragged: no frame starts aligned
    want = [crc16_ansi(data[off[i]:off[i + 1]]) for i in range(len(lens))]
    assert kern.crc16_frames(data, off) == want


# ------------------------------------------------------------------------------------------------------ stream contract
def _pcm(n, C=2, seed=5, fmt="s16le"):
    return synth.to_pcm(synth.harmonic_mix(n, C, 48000, seed=seed), fmt).tobytes()


def _encode(br, profile, pcm, ecc=None, overlap=0, le=False, bits=16, fsize=512, fmt="s16le", cuts=(), C=2):
    enc = Encoder(profile, 48000, C, bits, fsize, fmt, bridge=br, allow_ecc=True, allow_profile2=profile == 2)
    enc.set_overlap_ratio(overlap)
    enc.set_little_endian(le)
    if ecc is not None:
        enc.set_ecc(True, ecc)
    out, prev = b"", 0
    for c in list(cuts) + [len(pcm)]:
        out += enc.process(pcm[prev:c]).buf
        prev = c
    return out + enc.flush().buf


def _frames(stream: bytes) -> list:
    """(header, payload) of every frame, force-flush headers as (header, None); walks the stream by offset (a header is at
    most 16 + 8 bytes), so a whole-length stream is parsed in linear time"""
    out, pos = [], 0
    while pos < len(stream):
        assert stream[pos:pos + 4] == b"\xff\xd0\xd2\x98"
        a = ASFH()
        state, _ = a.read(stream[pos:pos + 40])
        pos += a.header_bytes
        if state == "ForceFlush":
            out.append((a, None))
            continue
        assert state == "Complete"
        out.append((a, stream[pos:pos + a.frmbytes]))
        pos += a.frmbytes
    return out


def _expected(plain: bytes, ratio) -> bytes:
    """the unprotected stream's payloads through the host model, headers written by ASFH.write with ecc set (and the
    force-flush headers of the compact profiles with it too: the reference's ASFH.force_flush writes the ecc bit)"""
    dsize, cs = ratio
    out = []
    for a, frad in _frames(plain):
        if frad is None:
            a.ecc = True
            out.append(a.force_flush())
            continue
        assert not a.ecc
        a.ecc, a.ecc_dsize, a.ecc_codesize = True, dsize, cs
        out.append(a.write(rs_model(frad, dsize, cs)))
    return b"".join(out)


def _repaired(br, plain, ratio):
    """Repairer(ratio).process(plain) + flush(), with the ecc bit set in the force-flush headers: the Repairer copies a
    force-flush header as stored (ecc off in an unprotected stream), an encoder with ECC on writes it with the bit
    (tools/asfh.py force_flush) -- the one place where the two routes differ"""
    r = Repairer(ratio, bridge=br)
    out = []
    for a, frad in _frames(r.process(plain) + r.flush()):
        if frad is None:
            a.ecc = True
            out.append(a.force_flush())
        else:
            out.append(a.write(frad))
    return b"".join(out)


CASES = [  # profile, ratio, overlap, little endian
    (0, (96, 24), 0, False), (0, (223, 32), 2, True), (0, (16, 16), 16, False),
    (4, (96, 24), 0, True), (4, (1, 254), 0, False),
    (1, (96, 24), 2, False), (1, (223, 32), 16, True), (1, (16, 16), 0, False),
    (2, (96, 24), 16, False), (2, (5, 3), 2, False),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"p{c[0]}-{c[1][0]}.{c[1][1]}-o{c[2]}-{'le' if c[3] else 'be'}")
def test_stream_contract(br, case):
    profile, ratio, overlap, le = case
    fsize = 256 if profile in profiles.COMPACT else 300
    pcm = _pcm(5 * fsize + 77)
    rng = np.random.default_rng(profile * 10 + overlap)
    step = 4
    cuts = sorted({int(c) // step * step for c in rng.integers(1, len(pcm), 3)})
    plain = _encode(br, profile, pcm, None, overlap, le, fsize=fsize)
    prot = _encode(br, profile, pcm, ratio, overlap, le, fsize=fsize, cuts=cuts)
    assert prot == _repaired(br, plain, ratio)
    assert prot == _expected(plain, ratio)
    heads = [a for a, f in _frames(prot) if f is not None]
    assert heads and all(a.ecc and (a.ecc_dsize, a.ecc_codesize) == ratio for a in heads)


def test_profile0_payloads_are_the_oracle_s(br):
    """the independent expectation from the oracle itself: p0_analogue of every frame, the host model, ASFH.write"""
    from oracle import frad_oracle as fo
    fsize, C = 300, 2
    raw = _pcm(4 * fsize + 50, C)
    prot = _encode(br, 0, raw, (96, 24), fsize=fsize)
    x = np.frombuffer(raw, np.int16).reshape(-1, C)
    want = []
    for s in range(0, len(x), fsize):
        frame = fo.to_f64(x[s:s + fsize], fo.pcm_dtype("s16le"))
        frad, idx, ch, sr = fo.p0_analogue(frame, 16, 48000, False)
        a = ASFH()
        a.profile, a.ecc, a.ecc_dsize, a.ecc_codesize = 0, True, 96, 24
        a.bit_depth_index, a.channels, a.fsize, a.srate = idx, ch, len(frame), 48000
        want.append(a.write(rs_model(frad, 96, 24)))
    assert prot == b"".join(want)


@pytest.mark.parametrize("fmt", ["s8", "u8", "s16be", "s32le", "u32be", "f32le", "f64be"])
def test_every_pcm_format(br, fmt):
    pcm = _pcm(3 * 256 + 10, fmt=fmt)
    for profile in (0, 1):
        plain = _encode(br, profile, pcm, None, 0, False, fsize=256, fmt=fmt)
        assert _encode(br, profile, pcm, (17, 5), 0, False, fsize=256, fmt=fmt) == _repaired(br, plain, (17, 5))


def test_escalated_profile0_frames_are_protected(br):
    """a frame whose transform overflows the 16-bit storage float goes to a deeper format: frame-by-frame path, protected too"""
    x = synth.harmonic_mix(4 * 256, 2, 48000, seed=2)
    x[256:512] *= 1e6                                                    # one loud frame
    pcm = x.astype(">f8").tobytes()
    plain = _encode(br, 0, pcm, None, bits=16, fsize=256, fmt="f64be")
    depths = {a.bit_depth_index for a, f in _frames(plain) if f is not None}
    assert len(depths) > 1, "no frame escalated"
    prot = _encode(br, 0, pcm, (96, 24), bits=16, fsize=256, fmt="f64be")
    assert prot == _repaired(br, plain, (96, 24)) == _expected(plain, (96, 24))


def test_ecc_toggled_between_calls(br):
    for profile in (0, 1):
        fsize = 256
        pcm = _pcm(6 * fsize)
        enc = Encoder(profile, 48000, 2, 16, fsize, "s16le", bridge=br, allow_ecc=True)
        ref = Encoder(profile, 48000, 2, 16, fsize, "s16le", bridge=br)
        third = len(pcm) // 3 // 4 * 4
        for i, (on, ratio) in enumerate(((True, (96, 24)), (False, (96, 24)), (True, (20, 10)))):
            enc.set_ecc(on, ratio)
            chunk = pcm[i * third:(i + 1) * third] if i < 2 else pcm[2 * third:]
            got = enc.process(chunk).buf + (enc.flush().buf if i == 2 else b"")
            pl = ref.process(chunk).buf + (ref.flush().buf if i == 2 else b"")
            if on:
                assert got == _repaired(br, pl, ratio)
            else:                                                        # lossless headers keep the ratio bytes (asfh.py)
                assert _frames(got) and all(not a.ecc for a, _ in _frames(got))
                assert got == _expected_plain_with_ratio(pl, ratio)


def _expected_plain_with_ratio(plain: bytes, ratio) -> bytes:
    out = []
    for a, frad in _frames(plain):
        if frad is None:
            out.append(a.force_flush())
            continue
        a.ecc_dsize, a.ecc_codesize = ratio
        out.append(a.write(frad))
    return b"".join(out)


# ---------------------------------------------------------------------------------------------------------- round trip
def _decode(br, stream, fix=False):
    d = Decoder(fix, bridge=br)
    r = d.process(stream)
    f = d.flush()
    return np.concatenate([r.pcm, f.pcm]) if f.pcm.size else r.pcm


@pytest.mark.parametrize("profile", [0, 1])
def test_round_trip_and_repair(br, profile):
    fsize = 256
    pcm = _pcm(4 * fsize + 33)
    plain = _encode(br, profile, pcm, None, 2 if profile else 0, fsize=fsize)
    prot = _encode(br, profile, pcm, (96, 24), 2 if profile else 0, fsize=fsize)
    want = _decode(br, plain)
    assert np.array_equal(_decode(br, prot), want)
    # at most t = 12 byte errors in every 120-byte block of two frames' payloads
    rng = np.random.default_rng(4)
    damaged = bytearray(prot)
    pos = 0
    for i, (a, frad) in enumerate(_frames(prot)):
        head = a.header_bytes
        if frad is not None and i in (0, 2):
            for b0 in range(0, len(frad), 120):
                blk = min(120, len(frad) - b0)
                for p in rng.choice(blk, min(12, blk // 2), replace=False):
                    damaged[pos + head + b0 + int(p)] ^= int(rng.integers(1, 256))
        pos += head + (len(frad) if frad is not None else 0)
    assert bytes(damaged) != prot
    assert np.array_equal(_decode(br, bytes(damaged), fix=True), want)


# ------------------------------------------------------------------------------------------------------ opt-in discipline
def test_without_the_opt_in_set_ecc_still_refuses():
    enc = Encoder(0, 48000, 2, 16, 2048, "s16le", bridge=object())
    with pytest.raises(NotImplementedError):
        enc.set_ecc(True, (96, 24))
    enc.set_ecc(False, (0, 3))
    assert not enc.asfh.ecc and (enc.asfh.ecc_dsize, enc.asfh.ecc_codesize) == (96, 24)


def test_opt_in_set_ecc_is_the_reference_s(capsys):
    enc = Encoder(0, 48000, 2, 16, 2048, "s16le", bridge=object(), allow_ecc=True)
    enc.set_ecc(True, (200, 55))
    assert enc.asfh.ecc and (enc.asfh.ecc_dsize, enc.asfh.ecc_codesize) == (200, 55)
    assert capsys.readouterr().err == ""
    enc.set_ecc(True, (0, 10))
    assert (enc.asfh.ecc_dsize, enc.asfh.ecc_codesize) == (96, 24)
    assert capsys.readouterr().err == "ECC data size must not be zero\nSetting ECC to default 96 24\n"
    enc.set_ecc(True, (0, 256))
    assert capsys.readouterr().err == ("ECC data size must not be zero\n"
                                       "ECC data size and check size must not exceed 255, given: 0 and 256\n"
                                       "Setting ECC to default 96 24\n")
    enc.set_ecc(False, (200, 56))
    assert not enc.asfh.ecc and (enc.asfh.ecc_dsize, enc.asfh.ecc_codesize) == (96, 24)
    assert "must not exceed 255, given: 200 and 56" in capsys.readouterr().err
    p2 = Encoder(2, 48000, 2, 16, 2048, "s16le", bridge=object(), allow_ecc=True, allow_profile2=True)
    p2.set_ecc(True, (16, 16))
    assert p2.asfh.ecc


# ------------------------------------------------------------------------------------------------------- on the MI355X
@pytest.mark.gpu
def test_full_size_profile0_stream_matches_the_repairer_route():
    """cfg 2: 10 minutes of 48 kHz stereo through profile 0 at 32 bits, ECC (96, 24)"""
    from frad_python_amd.bridge import HipBridge
    br = HipBridge()
    n = 10 * 60 * 48000
    pcm = _pcm(n, seed=11)
    plain = _encode(br, 0, pcm, None, bits=32, fsize=2048)
    prot = _encode(br, 0, pcm, (96, 24), bits=32, fsize=2048)
    assert len(prot) > len(plain)
    assert prot == _repaired(br, plain, (96, 24))
