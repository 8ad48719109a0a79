"""Repairer and Decoder(fix_error=True) on whole streams (src/libfrad/repairer.py, decoder.py:63-68).  Byte contract: for a
stream written without ECC, Repairer(r).process(s) + flush() are the bytes the reference encoder writes with set_ecc(True, r)
-- the same headers with the ecc bit, dsize / codesize and the checksum of the protected payload, followed by ecc.encode of
the payload -- built here from the host model of tests/test_ecc.py and the package's own ASFH.write.
"emu": oracle arithmetic for the transform, the CPU interpreter of frad_ecc.hip for Reed-Solomon; "gpu": the MI355X."""
import numpy as np
import pytest

from frad_python_amd import Decoder, Encoder, Repairer, synth
from frad_python_amd.tools.asfh import ASFH
from test_ecc import EmuEcc, blocks_of, model_encode


class EmuStreamBridge:
    """OracleBridge (transform) + the interpreted Reed-Solomon kernels and native header scanner."""

    def __init__(self):
        from helpers import OracleBridge
        self.inner, self.rs = OracleBridge(), EmuEcc()
        self.scan_lib = self.rs.scan_lib
        self.rs_encode, self.rs_repair = self.rs.rs_encode, self.rs.rs_repair

    def __getattr__(self, name):
        return getattr(self.inner, name)


def _bridge(kind):
    if kind == "emu":
        return EmuStreamBridge()
    from frad_python_amd.bridge import HipBridge
    return HipBridge()


@pytest.fixture(params=[pytest.param("emu"), pytest.param("gpu", marks=pytest.mark.gpu)], scope="module")
def kind(request):
    return request.param


@pytest.fixture(scope="module")
def br(kind):
    return _bridge(kind)


STREAMS = {
    "p0": dict(profile=0, bits=16, fsize=512, overlap=0, n=1700),
    "p1": dict(profile=1, bits=16, fsize=256, overlap=4, n=1500),
    "p4": dict(profile=4, bits=24, fsize=300, overlap=0, n=1000),
}


def _encode(br, spec, seed=3):
    pcm = synth.to_pcm(synth.harmonic_mix(spec["n"], 2, 48000, seed=seed), "s16le").tobytes()
    enc = Encoder(spec["profile"], 48000, 2, spec["bits"], spec["fsize"], "s16le", bridge=br)
    enc.set_overlap_ratio(spec["overlap"])
    return enc.process(pcm).buf + enc.flush().buf


def _frames(br, stream):
    table, _, _ = br.scan_lib.asfh_scan(stream, 0)
    return table.tolist()


def _contract(br, stream, ratio):
    """what the reference encoder writes with set_ecc(True, ratio), from the unprotected stream"""
    out = []
    for (h_off, p_off, p_len, profile, ecc, le, depth, ch, srate, fsize, olap, _, _, fflush, crc) in _frames(br, stream):
        a = ASFH()
        a.profile, a.endian, a.bit_depth_index, a.channels, a.srate, a.fsize, a.overlap_ratio = profile, bool(le), depth, ch, srate, fsize, olap
        if fflush:
            out.append(a.force_flush())
            continue
        a.ecc, (a.ecc_dsize, a.ecc_codesize) = True, ratio
        out.append(a.write(model_encode(stream[p_off:p_off + p_len], *ratio)))
    return b"".join(out)


def _repair(br, stream, ratio, chunks=None):
    r = Repairer(ratio, bridge=br)
    if chunks is None:
        return r.process(stream) + r.process(b"") + r.flush()
    out, pos = [], 0
    for c in chunks:
        out.append(r.process(stream[pos:pos + c])); pos += c
    out.append(r.process(stream[pos:]))
    out.append(r.process(b""))
    return b"".join(out) + r.flush()


def _decode(br, stream, fix=False):
    d = Decoder(fix, bridge=br)
    res = d.process(stream)
    pcm = [res.pcm.reshape(-1, 2)] if res.pcm.size else []
    while True:                                   # force-flush headers end a process() call
        res = d.process(b"")
        if not res.pcm.size and not res.frames:
            break
        pcm.append(res.pcm.reshape(-1, 2))
    tail = d.flush().pcm
    if tail.size:
        pcm.append(tail.reshape(-1, 2))
    return np.concatenate(pcm) if pcm else np.zeros((0, 2))


def _damage_stream(br, stream, per_block, seed, first_block_only=False):
    """flip `per_block` bytes in every block (or only the first block) of every ECC frame's payload"""
    rng = np.random.default_rng(seed)
    s = bytearray(stream)
    for (h_off, p_off, p_len, profile, ecc, *_rest) in _frames(br, stream):
        dsize, csize = _rest[6], _rest[7]
        if not ecc or not p_len:
            continue
        bs = dsize + csize
        for b0 in range(0, p_len, bs):
            n = min(bs, p_len - b0)
            for p in rng.permutation(n)[:per_block]:
                s[p_off + b0 + int(p)] ^= int(rng.integers(1, 256))
            if first_block_only:
                break
    return bytes(s)


@pytest.mark.parametrize("name", list(STREAMS))
def test_repairer_byte_contract_and_decode(br, name):
    s = _encode(br, STREAMS[name])
    prot = _repair(br, s, (96, 24))
    assert prot == _contract(br, s, (96, 24))
    ref = _decode(br, s)
    assert np.array_equal(_decode(br, prot), ref)
    assert np.array_equal(_decode(br, prot, fix=True), ref)


@pytest.mark.parametrize("name", list(STREAMS))
def test_damage_within_t_is_repaired(br, name):
    s = _encode(br, STREAMS[name])
    prot = _repair(br, s, (96, 24))
    bad = _damage_stream(br, prot, 12, seed=len(name))
    assert bad != prot
    ref = _decode(br, s)
    assert np.array_equal(_decode(br, bad, fix=True), ref)
    assert _repair(br, bad, (96, 24)) == prot
    # without fix_error the check bytes are only stripped: the damage reaches the decoder
    if name != "p1":
        assert not np.array_equal(_decode(br, bad), ref)


def test_byte_wise_parser_repairs_too(br):
    """the decoder's byte-wise header parser (no native scanner) takes the same repair path"""
    s = _encode(br, STREAMS["p4"])
    bad = _damage_stream(br, _repair(br, s, (96, 24)), 5, seed=9)

    class NoScan:
        def __init__(self, inner):
            self.inner = inner

        def __getattr__(self, name):
            if name == "scan_lib":
                raise AttributeError(name)
            return getattr(self.inner, name)
    d = Decoder(True, bridge=NoScan(br))
    assert np.array_equal(d.process(bad).pcm.reshape(-1, 2), _decode(br, s))


def test_damage_beyond_t_zero_fills(br):
    """a block beyond repair becomes zero bytes: the repaired stream is the contract of the payload with that block zeroed"""
    s = _encode(br, STREAMS["p4"])
    prot = _repair(br, s, (96, 24))
    bad = _damage_stream(br, prot, 120, seed=4, first_block_only=True)     # every byte of every frame's first block
    zeroed = bytearray(s)
    for (h_off, p_off, p_len, *_r) in _frames(br, s):
        zeroed[p_off:p_off + min(96, p_len)] = bytes(min(96, p_len))
    # the zeroed stream's CRCs are stale, which ASFH.write in the contract recomputes from the payload
    assert _repair(br, bad, (96, 24)) == _contract(br, bytes(zeroed), (96, 24))
    fixed, cor, failed = br.rs_repair([prot[_frames(br, prot)[0][1]:][:120]], 96, 24)
    assert cor.tolist() == [0] and failed.tolist() == [0]


def test_idempotent_and_reratio(br):
    s = _encode(br, STREAMS["p0"])
    a = _repair(br, s, (96, 24))
    assert _repair(br, a, (96, 24)) == a
    b = _repair(br, a, (200, 50))
    assert b == _contract(br, s, (200, 50))
    assert _repair(br, b, (96, 24)) == a


def test_garbage_and_split_boundaries(br):
    s1, s2 = _encode(br, STREAMS["p0"]), _encode(br, STREAMS["p1"], seed=8)
    stream = b"junk-before" + s1 + b"\x00\xff\xd0 between" + s2 + b"tail"
    whole = _repair(br, stream, (96, 24))
    assert whole.startswith(b"junk-before") and whole.endswith(b"tail") and b"\x00\xff\xd0 between" in whole
    rng = np.random.default_rng(2)
    for _ in range(2):
        chunks = [int(c) for c in rng.integers(1, 700, 40)]
        assert _repair(br, stream, (96, 24), chunks) == whole


def test_invalid_ratio_falls_back_like_the_reference(br, capsys):
    assert Repairer((0, 10), bridge=br).ecc_ratio == (96, 24)
    err = capsys.readouterr().err.splitlines()
    assert err == ["ECC data size must not be zero", "Setting ECC to default 96 24"]
    assert Repairer((200, 100), bridge=br).ecc_ratio == (96, 24)
    err = capsys.readouterr().err.splitlines()
    assert err == ["ECC data size and check size must not exceed 255, given: 200 and 100", "Setting ECC to default 96 24"]
    assert Repairer((200, 55), bridge=br).ecc_ratio == (200, 55)


def test_api_surface():
    import frad_python_amd
    assert "Repairer" in frad_python_amd.__all__
    r = Repairer(bridge=object())
    assert r.ecc_ratio == (96, 24) and r.is_empty() and r.flush() == b""
    Decoder(fix_error=True, bridge=object())                 # no longer refused


@pytest.mark.gpu
def test_full_size_profile0_stream():
    """a cfg-2-sized stream (14 062 frames of 2048 x 2 at 64 bits) through Repairer and Decoder(fix_error=True)"""
    import torch
    from frad_python_amd.bridge import HipBridge
    br = HipBridge()
    N, C, F = 2048, 2, 14062
    g = torch.Generator().manual_seed(5)
    pcm = (torch.randn(F * N, C, generator=g) * 3000).to(torch.int16).numpy().tobytes()
    enc = Encoder(0, 48000, C, 64, N, "s16le", bridge=br)
    s = enc.process(pcm).buf + enc.flush().buf
    prot = _repair(br, s, (96, 24))
    rows = _frames(br, prot)
    assert len(rows) == F
    bad = bytearray(prot)
    rng = np.random.default_rng(1)
    for i in rng.choice(F, 300, replace=False):                 # scattered damage, up to t bytes in a block
        p_off, p_len = rows[i][1], rows[i][2]
        b0 = int(rng.integers(0, p_len // 120)) * 120
        for p in rng.permutation(120)[:int(rng.integers(1, 13))]:
            bad[p_off + b0 + int(p)] ^= int(rng.integers(1, 256))
    bad = bytes(bad)
    assert _repair(br, bad, (96, 24)) == prot
    ref = Decoder(bridge=br).process(s).pcm
    assert np.array_equal(Decoder(True, bridge=br).process(bad).pcm, ref)
    assert blocks_of(prot[rows[0][1]:rows[0][1] + 120], 120)[0].size == 120
