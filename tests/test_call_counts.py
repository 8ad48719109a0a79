"""The C-ABI calls each streaming operation makes, by name and number, pinned.

test_batch_decode only compares the counts of 8 clips with those of 64; nothing else says what one operation costs.  The
numbers below were recorded on the commit before the operator layer was rebuilt (binding generated from ``_lib.SYMBOLS``,
pointers and streams in core.py only) and must not move without a reason: one more ``rows_compact`` or ``payload_bytes`` per
call is a launch or a host round trip per batch.

Every input is 48 kHz ``s16le``, a seeded ``synth.harmonic_mix`` of four whole frames of N = 128 and a short tail (128 is a
legal frame size of every profile used here)."""
import pytest

from frad_python_amd import Decoder, Encoder, Repairer, _lib, decode_batch, synth
from test_batch_decode import Counting

pytestmark = pytest.mark.gpu

N, SRATE, TAIL = 128, 48000, 50
RATIO = (96, 24)

# name: (profile, channels, overlap ratio, Encoder keywords, ECC)
ENCODERS = {
    "p0": (0, 1, 0, {}, False),
    "p0_ecc": (0, 1, 0, {"allow_ecc": True}, True),
    "p1": (1, 2, 2, {}, False),
    "p1_device_deflate": (1, 2, 2, {"device_deflate": True}, False),
    "p1_ecc": (1, 2, 2, {"allow_ecc": True}, True),
    "p2": (2, 2, 2, {"allow_profile2": True}, False),
}
# name: (stream, Decoder keywords)
DECODERS = {
    "p0": ("p0", {}),
    "p0_ecc": ("p0_ecc", {}),
    "p1": ("p1", {}),
    "p1_device_inflate": ("p1", {"device_inflate": True}),
    "p1_fix_error": ("p1", {"fix_error": True}),
    "p1_device_deflate": ("p1_device_deflate", {}),
    "p1_ecc": ("p1_ecc", {}),
    "p2": ("p2", {}),
}
BATCH = ("p0", "p1", "p2")

EXPECTED = {
    "decode_batch": {"asfh_scan": 1, "clips_overlap_add": 3, "p0_digital": 3, "p1_digital": 1, "p1_golomb_decode": 1, "p2_golomb_decode": 1, "p2_synth": 1, "payload_bytes": 3},
    "decode_p0": {"asfh_scan": 2, "p0_digital": 2, "payload_bytes": 3},
    "decode_p0_ecc": {"asfh_scan": 2, "p0_digital": 2, "payload_bytes": 2},
    "decode_p1": {"asfh_scan": 2, "p1_digital": 1, "p1_golomb_decode": 1, "p1_overlap_add": 1},
    "decode_p1_device_deflate": {"asfh_scan": 2, "p1_digital": 1, "p1_golomb_decode": 1, "p1_overlap_add": 1},
    "decode_p1_device_inflate": {"asfh_scan": 2, "inflate_raw": 1, "p1_digital": 1, "p1_golomb_bound": 1, "p1_golomb_decode": 1, "p1_overlap_add": 1, "rows_compact": 2},
    "decode_p1_ecc": {"asfh_scan": 2, "p1_digital": 1, "p1_golomb_decode": 1, "p1_overlap_add": 1},
    "decode_p1_fix_error": {"asfh_scan": 2, "p1_digital": 1, "p1_golomb_decode": 1, "p1_overlap_add": 1},
    "decode_p2": {"asfh_scan": 2, "p0_digital": 1, "p1_overlap_add": 1, "p2_golomb_decode": 1, "p2_synth": 1, "payload_bytes": 1},
    "encode_p0": {"crc32_frames": 1, "p0_analogue": 2, "payload_bytes": 3},
    "encode_p0_ecc": {"crc32_frames": 2, "p0_analogue": 2, "payload_bytes": 3, "rs_encode": 1, "rs_encode_frames": 1},
    "encode_p1": {"p1_analogue": 2, "p1_golomb_bound": 2, "p1_golomb_encode": 2, "rows_compact": 4},
    "encode_p1_device_deflate": {"deflate_raw": 2, "deflate_stride": 2, "p1_analogue": 2, "p1_golomb_bound": 2, "p1_golomb_encode": 2, "rows_compact": 8},
    "encode_p1_ecc": {"crc16_ansi_frames": 2, "p1_analogue": 2, "p1_golomb_bound": 2, "p1_golomb_encode": 2, "rows_compact": 4, "rs_encode": 2},
    "encode_p2": {"p2_analogue": 2, "p2_golomb_bound": 2, "p2_golomb_encode": 2, "rows_compact": 4},
    "repair_p0": {"asfh_scan": 1, "crc32_frames": 2, "rs_encode": 1},
}


def pcm(channels: int) -> bytes:
    return synth.to_pcm(synth.harmonic_mix(4 * N + TAIL, channels, SRATE, seed=20 + channels), "s16le").tobytes()


def encode(name: str, bridge=None) -> bytes:
    profile, channels, overlap, kw, ecc = ENCODERS[name]
    enc = Encoder(profile, SRATE, channels, 16, N, "s16le", bridge=bridge, **kw)
    enc.set_overlap_ratio(overlap)
    if ecc:
        enc.set_ecc(True, RATIO)
    return enc.process(pcm(channels)).buf + enc.flush().buf


_streams = {}


def stream(name: str) -> bytes:
    if name not in _streams:
        _streams[name] = encode(name)
    return _streams[name]


def decode(name: str, bridge):
    src, kw = DECODERS[name]
    dec = Decoder(bridge=bridge, **kw)
    return [dec.process(stream(src)), dec.process(b""), dec.flush()]


def scenarios():
    """name -> (the streams it needs made beforehand, the operation, given a bridge)"""
    out = {f"encode_{k}": ((), lambda br, k=k: encode(k, br)) for k in ENCODERS}
    out.update({f"decode_{k}": ((v[0],), lambda br, k=k: decode(k, br)) for k, v in DECODERS.items()})
    out["repair_p0"] = (("p0",), lambda br: Repairer(RATIO, bridge=br).process(stream("p0")))
    out["decode_batch"] = (BATCH, lambda br: decode_batch([stream(k) for k in BATCH], bridge=br))
    return out


def count_calls(name: str, monkeypatch) -> dict:
    """every C-ABI call of the loaded library while the scenario runs, name -> count"""
    from frad_python_amd.bridge import HipBridge
    needs, run = scenarios()[name]
    for k in needs:
        stream(k)
    counts = {}
    monkeypatch.setattr(_lib, "_lib", Counting(_lib.load(), counts))
    try:
        run(HipBridge())
    finally:
        monkeypatch.undo()
    return counts


@pytest.mark.parametrize("name", sorted(scenarios()))
def test_an_operation_makes_the_recorded_calls(name, monkeypatch):
    got = count_calls(name, monkeypatch)
    print(f"[calls] {name}: {dict(sorted(got.items()))}")
    assert got == EXPECTED[name]
