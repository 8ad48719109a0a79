"""Batched operators of the transform core on PyTorch-ROCm tensors.

One call = one HIP launch over ``n_frames`` independent frames (the reference runs one frame
per call through ``fourier.profileN.analogue/digital``, src/libfrad/encoder.py:96-100 and
decoder.py:70-74).  Tensors only carry device memory and the current stream into the C-ABI
(include/frad_hip.h); all arithmetic happens in libfrad_hip.so.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, ecc
from .backend.pcmformat import itemsize_of, pcm_dtype_code

DEPTHS = (12, 16, 24, 32, 48, 64)                      # ref: fourier/profile0.py:4, profile4.py:4
# largest finite value of each depth's storage float (ref: profile0.py:6-13 FLOAT_DR)
FLOAT_MAX = {12: 65504.0, 16: 65504.0, 24: float(np.finfo("f4").max), 32: float(np.finfo("f4").max),
             48: float(np.finfo("f8").max), 64: float(np.finfo("f8").max)}
_ESCALATE = {12: 16, 16: 24, 24: 32, 32: 48, 48: 64, 64: 128}


def _require_cuda(t: torch.Tensor, what: str, contiguous: bool = True):
    if not t.is_cuda:
        raise RuntimeError(f"{what} must live in MI355X device memory (got a {t.device} tensor); "
                           "the transform core has no CPU path")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def _stream_ptr() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def _align16(n: int) -> int:
    return (n + 15) // 16 * 16


def payload_bytes(N: int, C: int, bits: int) -> int:
    """bytes of one profile-0 / 4 payload (frad_payload_bytes)"""
    return _lib.load().payload_bytes(N, C, bits)


def _require_pcm_span(pcm: torch.Tensor, n_frames: int, hop: int, n_valid: int, C: int, code: int):
    """frame i reads ``n_valid`` sample-frames of C elements, ``i * hop`` sample-frames into ``pcm``: the last one must end inside it"""
    need = ((n_frames - 1) * hop + n_valid) * C * itemsize_of(code) if n_frames else 0
    if pcm.numel() * pcm.element_size() < need:
        raise ValueError(f"pcm holds {pcm.numel() * pcm.element_size()} bytes, {need} needed")


def _clip_frames(clip_len: int, N: int, first: int, frames_per_clip: int | None) -> int:
    """frames of N sample-frames per clip from ``first`` on (default: as many whole ones as fit)"""
    fpc = (clip_len - first) // N if frames_per_clip is None else frames_per_clip
    if fpc < 1 or first < 0 or first + fpc * N > clip_len:
        raise ValueError("the frames do not fit the clip")
    return fpc


def _p0_encode_buffers(lib, n_frames: int, N: int, C: int, bits: int, little_endian: bool, raw_be_ints: bool, out, absmax, device):
    """What the two profile-0 encoders settle before the launch -> (bits, nbytes, flags, out, absmax): the depth default,
    the flag word, and ``out`` uint8 [n_frames, align16(nbytes)] / ``absmax`` float64 [n_frames] where the caller brought none."""
    if bits not in DEPTHS:
        bits = 16                                         # ref: profile0.py:15
    nbytes = lib.payload_bytes(N, C, bits)
    if out is None:
        out = torch.empty((n_frames, _align16(nbytes)), dtype=torch.uint8, device=device)
    if absmax is None:
        absmax = torch.empty(n_frames, dtype=torch.float64, device=device)
    flags = (int(little_endian) * _lib.FRAD_LITTLE_ENDIAN) | (int(raw_be_ints) * _lib.FRAD_RAW_BE_INTS)
    return bits, nbytes, flags, out, absmax


def escalate_depth(absmax: float, bits: int) -> int:
    """The reference's overflow loop (profile0.py:24-26): NaN never escalates, +Inf raises."""
    while absmax > FLOAT_MAX[bits]:
        bits = _ESCALATE[bits]
        if bits == 128:
            raise OverflowError("Overflow with reaching the max bit depth.")
    return bits


@dataclass
class EncodedBatch:
    """Payloads of one batched ``analogue`` call.

    ``payload[i, :nbytes]`` is frame i at the requested depth.  A frame whose transform exceeds the
    storage float's range (profile0.py:24-26) is listed in ``escalated`` as
    ``{frame: (payload_row_tensor, bits)}`` at the deeper format the reference would pick."""
    payload: torch.Tensor            # uint8 [n_frames, stride]
    nbytes: int
    bits: int
    absmax: torch.Tensor             # float64 [n_frames]
    escalated: dict

    def frame_bytes(self, i: int) -> tuple[bytes, int]:
        if i in self.escalated:
            row, bits = self.escalated[i]
            return bytes(row.cpu().numpy()), bits
        return bytes(self.payload[i, :self.nbytes].cpu().numpy()), self.bits


def analogue_batch(profile: int, pcm: torch.Tensor, pcm_format: str, n_frames: int, N: int, C: int, bits: int,
                   little_endian: bool = False, *, frame_stride: int | None = None, raw_be_ints: bool = True,
                   check_overflow: bool = True, out: torch.Tensor | None = None,
                   absmax: torch.Tensor | None = None, overflow_flag: torch.Tensor | None = None) -> EncodedBatch:
    """Profile 0 (DCT) or 4 (PCM) ``analogue`` over a batch of frames.

    ``pcm`` is the raw interleaved PCM (any tensor dtype; ``pcm_format`` names the element type as
    the reference's CLI does, e.g. ``s16le``), frame i starting ``frame_stride`` (default N)
    sample-frames after frame i-1.  ``overflow_flag`` (profile 0, device int32 scalar): the batch form of the reference's
    overflow test in the same pass -- set to 1 when a frame needs a deeper format, read it when the answer is needed."""
    _require_cuda(pcm, "pcm")
    lib = _lib.load()
    code = pcm_dtype_code(pcm_format)
    stride_frames = N if frame_stride is None else frame_stride
    _require_pcm_span(pcm, n_frames, stride_frames, N, C, code)
    bits, nbytes, flags, out, absmax = _p0_encode_buffers(lib, n_frames, N, C, bits, little_endian, raw_be_ints, out, absmax, pcm.device)
    fn = lib.p4_analogue if profile == 4 else lib.p0_analogue
    with torch.cuda.device(pcm.device):
        if overflow_flag is not None and profile != 4:
            _require_cuda(overflow_flag, "overflow_flag")
            if overflow_flag.dtype != torch.int32:
                raise TypeError("overflow_flag must be int32")
            lib.p0_analogue_checked(pcm.data_ptr(), code, n_frames, N, C, stride_frames, bits, flags, out.data_ptr(), out.stride(0),
                                    absmax.data_ptr(), overflow_flag.data_ptr(), _stream_ptr())
        else:
            fn(pcm.data_ptr(), code, n_frames, N, C, stride_frames, bits, flags, out.data_ptr(), out.stride(0),
               absmax.data_ptr(), _stream_ptr())
    escalated = {}
    if check_overflow and n_frames:
        over = absmax > FLOAT_MAX[bits]                   # NaN compares False, as in the reference
        idx = over.nonzero().flatten()                    # (one host sync: the number of offenders sizes the re-dispatch)
        if idx.numel():
            # the offenders again, one launch per deeper format the reference's loop would settle on (profile0.py:24-26)
            isz = itemsize_of(code)
            flat = pcm.reshape(-1).view(torch.uint8)
            frame_bytes_n = N * C * isz
            byte_idx = torch.arange(frame_bytes_n, device=pcm.device)
            am_host = absmax[idx].cpu().tolist()
            by_depth: dict[int, list[int]] = {}
            for i, a in zip(idx.tolist(), am_host):
                by_depth.setdefault(escalate_depth(float(a), bits), []).append(i)
            for deeper, frames in by_depth.items():
                starts = torch.tensor(frames, device=pcm.device, dtype=torch.int64) * (stride_frames * C * isz)
                gathered = flat[(starts[:, None] + byte_idx[None, :]).reshape(-1)]     # [len(frames), N*C*isz] contiguous
                sub = analogue_batch(profile, gathered, pcm_format, len(frames), N, C, deeper, little_endian,
                                     raw_be_ints=raw_be_ints, check_overflow=False)
                for j, i in enumerate(frames):
                    escalated[i] = (sub.payload[j, :sub.nbytes], deeper)
    return EncodedBatch(out, nbytes, bits, absmax, escalated)


def analogue_clips(clips: torch.Tensor, pcm_format: str, N: int, bits: int, little_endian: bool = False, *,
                   first: int = 0, frames_per_clip: int | None = None, raw_be_ints: bool = True,
                   out: torch.Tensor | None = None, absmax: torch.Tensor | None = None,
                   overflow_flag: torch.Tensor | None = None) -> EncodedBatch:
    """Profile 0 ``analogue`` over a resident batch of equally long clips ``[n_clips, clip_len, C]``, consumed in place
    (frad_p0_analogue_clips; the reference cuts every clip into frames on its own, encoder.py:72-93): ``frames_per_clip``
    frames of N sample-frames per clip, the first one ``first`` sample-frames into the clip (default: as many whole
    frames as fit behind ``first``).  A clip's shorter last frame is a second call with its own N and ``first``.
    Payload row ``c * frames_per_clip + i`` is frame i of clip c.  The overflow test is the device flag only."""
    _require_cuda(clips, "clips")
    if clips.dim() != 3:
        raise ValueError("clips must be [n_clips, clip_len, C]")
    lib = _lib.load()
    code = pcm_dtype_code(pcm_format)
    n_clips, clip_len, C = clips.shape
    if clips.element_size() != itemsize_of(code):
        raise ValueError("clips' element size does not match pcm_format")
    fpc = _clip_frames(clip_len, N, first, frames_per_clip)
    bits, nbytes, flags, out, absmax = _p0_encode_buffers(lib, n_clips * fpc, N, C, bits, little_endian, raw_be_ints, out, absmax,
                                                          clips.device)
    with torch.cuda.device(clips.device):
        lib.p0_analogue_clips(clips.data_ptr() + first * C * clips.element_size(), code, n_clips, clip_len, fpc, N, C, bits, flags,
                              out.data_ptr(), out.stride(0), absmax.data_ptr(),
                              overflow_flag.data_ptr() if overflow_flag is not None else 0, _stream_ptr())
    return EncodedBatch(out, nbytes, bits, absmax, {})


def digital_clips(payload: torch.Tensor, out: torch.Tensor, N: int, bits: int, little_endian: bool = False, *,
                  first: int = 0, frames_per_clip: int | None = None) -> torch.Tensor:
    """Profile 0 ``digital`` of a clip batch straight into ``out`` = float64 ``[n_clips, clip_len, C]`` (frad_p0_digital_clips):
    payload row ``c * frames_per_clip + i`` lands at ``out[c, first + i*N : first + (i+1)*N]``."""
    _require_cuda(payload, "payload"); _require_cuda(out, "out")
    if out.dim() != 3 or out.dtype != torch.float64:
        raise ValueError("out must be float64 [n_clips, clip_len, C]")
    lib = _lib.load()
    n_clips, clip_len, C = out.shape
    fpc = _clip_frames(clip_len, N, first, frames_per_clip)
    if payload.shape[0] < n_clips * fpc:
        raise ValueError("the frames do not fit the payload batch")
    flags = int(little_endian) * _lib.FRAD_LITTLE_ENDIAN
    with torch.cuda.device(out.device):
        lib.p0_digital_clips(payload.data_ptr(), payload.stride(0), n_clips, fpc, N, C, bits, flags,
                             out.data_ptr() + first * C * 8, clip_len, _stream_ptr())
    return out


def overflow_scan(absmax: torch.Tensor, bits: int, flag: torch.Tensor) -> None:
    """``flag |= any(absmax > FLOAT_MAX[bits])`` in one launch (profile0.py:24-26 over a batch).

    ``flag`` is a device int32 scalar kept across batches; read it when the answer is needed."""
    _require_cuda(absmax, "absmax"); _require_cuda(flag, "flag")
    if absmax.dtype != torch.float64 or flag.dtype != torch.int32:
        raise TypeError("absmax must be float64 and flag int32")
    with torch.cuda.device(absmax.device):
        _lib.load().p0_overflow_scan(absmax.data_ptr(), absmax.numel(), bits, flag.data_ptr(), _stream_ptr())


def crc32_frames(payload: torch.Tensor, nbytes: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """zlib.crc32 of ``payload[i, :nbytes]`` for every row, as int32 bit patterns on the device
    (the checksum ASFH.write stores in a lossless frame header, tools/asfh.py:51-73); into ``out`` int32 [n_frames] if given."""
    _require_cuda(payload, "payload", contiguous=False)
    if payload.dtype != torch.uint8 or payload.dim() != 2 or payload.stride(1) != 1 or payload.shape[1] < nbytes:
        raise ValueError("payload must be a uint8 [n_frames, >= nbytes] tensor with unit column stride")
    if out is None:
        out = torch.empty(payload.shape[0], dtype=torch.int32, device=payload.device)
    elif out.dtype != torch.int32 or out.shape != payload.shape[:1] or out.device != payload.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous int32 [{payload.shape[0]}] tensor on {payload.device}")
    with torch.cuda.device(payload.device):
        _lib.load().crc32_frames(payload.data_ptr(), payload.stride(0), payload.shape[0], nbytes, out.data_ptr(), _stream_ptr())
    return out


def rs_protected_bytes(nbytes: int, dsize: int, codesize: int) -> int:
    """length of ecc.encode of an ``nbytes`` payload: every dsize-byte chunk (the last may be shorter) gains codesize bytes"""
    return nbytes + -(-nbytes // dsize) * codesize


def _require_rs_ratio(dsize: int, codesize: int):
    if not (dsize >= 1 and codesize >= 0 and dsize + codesize <= 255):
        raise ValueError(f"Reed-Solomon ratio ({dsize}, {codesize}) outside 1 <= dsize, 0 <= codesize, dsize + codesize <= 255")


def _require_rows(t: torch.Tensor, width: int, what: str):
    _require_cuda(t, what, contiguous=False)
    if t.dtype != torch.uint8 or t.dim() != 2 or t.stride(1) != 1 or t.shape[1] < width or (t.shape[0] > 1 and t.stride(0) < width):
        raise ValueError(f"{what} must be a uint8 [n_frames, >= {width}] tensor with unit column stride and rows >= {width} bytes apart")


def rs_encode_frames(payload: torch.Tensor, nbytes: int, dsize: int, codesize: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """ecc.encode(payload[i, :nbytes], dsize, codesize) for every row (tools/ecc.py:6-12) into ``out[i, :P]``, P =
    ``rs_protected_bytes(nbytes, ...)``; ``out`` may be a strided view (e.g. the payload columns of a stream with header
    holes) and nothing else of it is written.  -> out[:, :P]"""
    _require_rs_ratio(dsize, codesize)
    if nbytes < 0:
        raise ValueError("nbytes must be >= 0")
    _require_rows(payload, nbytes, "payload")
    P = rs_protected_bytes(nbytes, dsize, codesize)
    if out is None:
        out = torch.empty((payload.shape[0], _align16(P)), dtype=torch.uint8, device=payload.device)
    _require_rows(out, P, "out")
    if out.shape[0] != payload.shape[0] or out.device != payload.device:
        raise ValueError(f"out must hold {payload.shape[0]} rows on {payload.device}")
    with torch.cuda.device(payload.device):
        _lib.load().rs_encode_frames(payload.data_ptr(), payload.stride(0), payload.shape[0], nbytes, dsize, codesize,
                                     out.data_ptr(), out.stride(0), _stream_ptr())
    return out[:, :P]


def _require_ragged(src: torch.Tensor, offsets: torch.Tensor, what: str) -> int:
    """The static half of a ragged batch's check -- ``src`` uint8 [total] and ``offsets`` int64 [n_frames + 1], contiguous on
    one device, frame i at ``src[offsets[i]:offsets[i + 1]]`` -- without looking at a value.  -> n_frames"""
    _require_cuda(src, what); _require_cuda(offsets, "offsets")
    if src.dtype != torch.uint8 or src.dim() != 1:
        raise ValueError(f"{what} must be a 1-D uint8 tensor (got {src.dtype} {list(src.shape)})")
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1 or offsets.device != src.device:
        raise ValueError(f"offsets must be a 1-D int64 tensor of n_frames + 1 entries on the device of {what}")
    return offsets.numel() - 1


def _require_offsets_within(src: torch.Tensor, offsets: torch.Tensor, *more) -> list:
    """The other half: the offsets do not decrease and stay within ``src``, so no caller buffer reaches a kernel unchecked.
    This is the operator's one device-to-host read; ``more`` (0-d int64 tensors) ride along and come back as integers."""
    lo, hi, mono, *more = torch.stack([offsets.min(), offsets.max(), (offsets[1:] < offsets[:-1]).any().to(torch.int64), *more]).tolist()
    if lo < 0 or hi > src.numel() or mono:
        raise ValueError(f"offsets must be non-decreasing and within [0, {src.numel()}] (got min {lo}, max {hi})")
    return more


def _require_frame_count(n_frames: int, what: str):
    if n_frames > 0x7fffffff:
        raise ValueError(f"at most 2^31 - 1 {what} per batch")


def _rs_pointers(packed: torch.Tensor, head: int, n_frames: int) -> list:
    _require_cuda(packed, "packed")
    return [packed.data_ptr() + o for o in ecc.pack_layout(head, n_frames)]


def rs_encode_packed(packed: torch.Tensor, head: int, n_frames: int, n_blocks: int, dsize: int, codesize: int, out: torch.Tensor):
    """frad_rs_encode over ``packed``, the uploaded buffer of ``ecc.pack(payloads, dsize, codesize, False)`` (``head``,
    ``n_blocks`` as it returned them): ecc.encode of payload i to ``out[out_off[i]:out_off[i + 1]]`` (uint8, contiguous)."""
    _require_cuda(out, "out")
    with torch.cuda.device(packed.device):
        _lib.load().rs_encode(*_rs_pointers(packed, head, n_frames), n_frames, n_blocks, dsize, codesize, out.data_ptr(), _stream_ptr())
    return out


def rs_repair_packed(packed: torch.Tensor, head: int, n_frames: int, n_blocks: int, dsize: int, codesize: int, out: torch.Tensor):
    """frad_rs_repair over the uploaded ``ecc.pack(payloads, dsize, codesize, True)``: the repaired data part of payload i to
    ``out[out_off[i]:out_off[i + 1]]``.  -> int32 [2 * n_frames]: corrected blocks per payload, then failed blocks per payload"""
    _require_cuda(out, "out")
    counts = torch.empty(2 * n_frames + n_blocks + 1, dtype=torch.int32, device=packed.device)    # corrected, failed, work list
    c = counts.data_ptr()
    with torch.cuda.device(packed.device):
        _lib.load().rs_repair(*_rs_pointers(packed, head, n_frames), n_frames, n_blocks, dsize, codesize, out.data_ptr(),
                              c, c + 4 * n_frames, c + 8 * n_frames, _stream_ptr())
    return counts[:2 * n_frames]


def crc16_ansi_frames(data: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """common.crc16_ansi of ``data[offsets[i]:offsets[i + 1]]`` for every frame, as int16 bit patterns on the device (the
    checksum a compact-profile ECC header stores, tools/asfh.py).  The offsets are checked against ``data`` before the launch
    (one small device-to-host read)."""
    n = _require_ragged(data, offsets, "data")
    _require_offsets_within(data, offsets)
    out = torch.empty(n, dtype=torch.int16, device=data.device)
    with torch.cuda.device(data.device):
        _lib.load().crc16_ansi_frames(data.data_ptr(), offsets.data_ptr(), n, out.data_ptr(), _stream_ptr())
    return out


def _pcm_out_tensor(fmt: str, shape, device, slack: int = 0) -> torch.Tensor:
    """uint8 storage for `shape` elements of PCM format `fmt` (torch has no big-endian or unsigned 16/32/64 dtypes), with
    ``slack`` allocated bytes behind it that the tensor does not show"""
    n = itemsize_of(pcm_dtype_code(fmt))
    for d in shape:
        n *= d
    return torch.empty(n + slack, dtype=torch.uint8, device=device)[:n] if slack else torch.empty(n, dtype=torch.uint8, device=device)


def from_f64(pcm: torch.Tensor, out_format: str, *, raw_be_ints: bool = True) -> torch.Tensor:
    """``from_f64(pcm, fmt).astype(fmt)`` as the reference's caller applies it to decoded blocks (pcmformat.py:49-62,
    src/decoder.py:23): float64 tensor -> the bytes of PCM format ``out_format`` (uint8 tensor)."""
    _require_cuda(pcm, "pcm")
    if pcm.dtype != torch.float64 or not pcm.is_contiguous():
        raise TypeError("pcm must be contiguous float64")
    out = _pcm_out_tensor(out_format, pcm.shape, pcm.device)
    with torch.cuda.device(pcm.device):
        _lib.load().from_f64(pcm.data_ptr(), pcm.numel(), pcm_dtype_code(out_format), out.data_ptr(), _stream_ptr(),
                             int(raw_be_ints) * _lib.FRAD_RAW_BE_INTS)
    return out


def digital_batch(profile: int, payload: torch.Tensor, n_frames: int, N: int, C: int, bits: int,
                  little_endian: bool = False, *, payload_stride: int | None = None,
                  out: torch.Tensor | None = None, out_format: str | None = None) -> torch.Tensor:
    """Profile 0 / 4 ``digital`` over a batch: uint8 payload rows -> float64 [n_frames, N, C]; with ``out_format`` the
    samples leave the device already narrowed to that PCM format (uint8 tensor of its bytes, see ``from_f64``)."""
    _require_cuda(payload, "payload")
    lib = _lib.load()
    nbytes = lib.payload_bytes(N, C, bits)
    if payload_stride is None:
        payload_stride = payload.stride(0) if payload.dim() == 2 else nbytes
    if payload.numel() * payload.element_size() < ((n_frames - 1) * payload_stride + nbytes if n_frames else 0):
        raise ValueError("payload tensor is smaller than n_frames frames")
    flags = int(little_endian) * _lib.FRAD_LITTLE_ENDIAN
    if out_format is not None:
        flags |= _lib.FRAD_RAW_BE_INTS                          # the reference's from_f64 does not recognise big-endian ints
        if out is None:
            out = _pcm_out_tensor(out_format, (n_frames, N, C), payload.device)
        fn = lib.p4_digital_pcm if profile == 4 else lib.p0_digital_pcm
        with torch.cuda.device(payload.device):
            fn(payload.data_ptr(), payload_stride, n_frames, N, C, bits, flags, pcm_dtype_code(out_format), out.data_ptr(), _stream_ptr())
        return out
    if out is None:
        out = torch.empty((n_frames, N, C), dtype=torch.float64, device=payload.device)
    fn = lib.p4_digital if profile == 4 else lib.p0_digital
    with torch.cuda.device(payload.device):
        fn(payload.data_ptr(), payload_stride, n_frames, N, C, bits, flags, out.data_ptr(), _stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------
# profile 1 (psychoacoustic quantiser): the integer arrays either side of the host entropy coder
# ---------------------------------------------------------------------------------------------
P1_DEPTHS = (8, 12, 16, 24, 32, 48, 64)                # ref: fourier/profile1.py:7
P1_BANDS = 27


def p1_analogue_batch(pcm: torch.Tensor, pcm_format: str, n_frames: int, N: int, C: int, bits: int, srate: int,
                      loss_level: float, *, frame_stride: int | None = None, n_valid: int | None = None,
                      raw_be_ints: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
    """``profile1.analogue`` up to the Exp-Golomb coder (profile1.py:15-40), batched.

    Frame i reads ``n_valid`` (default N) sample-frames at ``pcm + i*frame_stride`` (the hop when the
    encoder overlaps) and is zero-padded to the compact frame size N.  Returns ``q`` int32
    [n_frames, N, C] and ``tq`` int32 [n_frames, 27, C]."""
    _require_cuda(pcm, "pcm")
    lib = _lib.load()
    code = pcm_dtype_code(pcm_format)
    hop = N if frame_stride is None else frame_stride
    nv = N if n_valid is None else n_valid
    _require_pcm_span(pcm, n_frames, hop, nv, C, code)
    q = torch.empty((n_frames, N, C), dtype=torch.int32, device=pcm.device)
    tq = torch.empty((n_frames, P1_BANDS, C), dtype=torch.int32, device=pcm.device)
    flags = int(raw_be_ints) * _lib.FRAD_RAW_BE_INTS
    with torch.cuda.device(pcm.device):
        lib.p1_analogue(pcm.data_ptr(), code, n_frames, N, C, hop, nv, bits, srate, float(loss_level), flags,
                        q.data_ptr(), tq.data_ptr(), _stream_ptr())
    return q, tq


def golomb_bound(profile: int, N: int, C: int) -> int:
    """upper bound of one frame's pre-deflate body, a multiple of 16 (frad_p1_golomb_bound / frad_p2_golomb_bound)"""
    lib = _lib.load()
    return lib.p1_golomb_bound(N, C) if profile == 1 else lib.p2_golomb_bound(N, C)


def rows_offsets(rows: torch.Tensor, nbytes: torch.Tensor) -> torch.Tensor:
    """The scan pass of frad_rows_compact: ``rows`` uint8 [n, stride] of which row i holds ``nbytes[i]`` (int64) bytes ->
    ``offsets`` int64 [n + 1], the rows' places when laid back to back; ``offsets[-1]`` (for the caller to read) is their total."""
    n, stride = rows.shape
    offsets = torch.empty(n + 1, dtype=torch.int64, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.load().rows_compact(rows.data_ptr(), stride, nbytes.data_ptr(), n, 0, offsets.data_ptr(), _stream_ptr())
    return offsets


def rows_gather(rows: torch.Tensor, nbytes: torch.Tensor, offsets: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """The gather pass of frad_rows_compact: row i's bytes to ``out[offsets[i]:offsets[i + 1]]``, ``offsets`` from
    ``rows_offsets`` and ``out`` a contiguous uint8 tensor of at least ``offsets[-1]`` bytes (the caller has read the total)."""
    n, stride = rows.shape
    with torch.cuda.device(rows.device):
        _lib.load().rows_compact(rows.data_ptr(), stride, nbytes.data_ptr(), n, out.data_ptr(), offsets.data_ptr(), _stream_ptr())
    return out


def _golomb_encode(profile: int, q: torch.Tensor, *ints) -> tuple[torch.Tensor, torch.Tensor]:
    """frad_p{1,2}_golomb_encode into rows of the bound's length, then the rows laid back to back -> (bodies, offsets)"""
    _require_cuda(q, "q")
    for t in ints:
        _require_cuda(t, "tq / lpc")
    n_frames, N, C = q.shape
    lib = _lib.load()
    stride = golomb_bound(profile, N, C)
    rows = torch.empty((n_frames, stride), dtype=torch.uint8, device=q.device)
    nbytes = torch.empty(n_frames, dtype=torch.int64, device=q.device)
    with torch.cuda.device(q.device):
        (lib.p1_golomb_encode if profile == 1 else lib.p2_golomb_encode)(
            q.data_ptr(), *(t.data_ptr() for t in ints), n_frames, N, C, rows.data_ptr(), stride, nbytes.data_ptr(), _stream_ptr())
    offsets = rows_offsets(rows, nbytes)
    total = int(offsets[-1].item()) if n_frames else 0      # the one host read: the size of the result
    return rows_gather(rows, nbytes, offsets, torch.empty(total, dtype=torch.uint8, device=q.device)), offsets


def p1_golomb_encode_batch(q: torch.Tensor, tq: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The Exp-Golomb-Rice stage of ``profile1.analogue`` (profile1.py:43-45, p1tools.py:46-60) on the device.

    ``q`` int32 [n_frames, N, C], ``tq`` int32 [n_frames, 27, C] -> ``(bodies uint8 [total], offsets int64
    [n_frames + 1])``: frame i's pre-deflate body ('>I' len + Golomb(tq) + Golomb(q)) is
    ``bodies[offsets[i]:offsets[i+1]]``.  Deflate stays on the host."""
    _require_cuda(q, "q"); _require_cuda(tq, "tq")
    if q.dtype != torch.int32 or tq.dtype != torch.int32 or not q.is_contiguous() or not tq.is_contiguous():
        raise TypeError("q and tq must be contiguous int32")
    return _golomb_encode(1, q, tq)


def p1_golomb_decode_batch(bodies: torch.Tensor, offsets: torch.Tensor, N: int, C: int):
    """The two ``exp_golomb_rice_decode`` calls + ``untrim`` of ``profile1.digital`` (profile1.py:59-64,
    p1tools.py:62-74): inflated bodies (uint8, frame i at ``offsets[i]:offsets[i+1]``) -> ``(q, tq, status)``."""
    n_frames = _require_ragged(bodies, offsets, "bodies")   # (no look at the values: that would be a host read in the decoder's run)
    q = torch.empty((n_frames, N, C), dtype=torch.int32, device=bodies.device)
    tq = torch.empty((n_frames, P1_BANDS, C), dtype=torch.int32, device=bodies.device)
    status = torch.empty(max(n_frames, 1), dtype=torch.int32, device=bodies.device)
    with torch.cuda.device(bodies.device):
        _lib.load().p1_golomb_decode(bodies.data_ptr(), offsets.data_ptr(), n_frames, N, C, q.data_ptr(), tq.data_ptr(),
                                     status.data_ptr(), _stream_ptr())
    return q, tq, status[:n_frames]


def p1_digital_batch(q: torch.Tensor, tq: torch.Tensor, N: int, C: int, bits: int, srate: int) -> torch.Tensor:
    """``profile1.digital`` from the decoded integers on (profile1.py:65-77): float64 [n_frames, N, C]."""
    _require_cuda(q, "q"); _require_cuda(tq, "tq")
    if q.dtype != torch.int32 or tq.dtype != torch.int32:
        raise TypeError("q and tq must be int32")
    n_frames = q.shape[0]
    out = torch.empty((n_frames, N, C), dtype=torch.float64, device=q.device)
    with torch.cuda.device(q.device):
        _lib.load().p1_digital(q.data_ptr(), tq.data_ptr(), n_frames, N, C, bits, srate, out.data_ptr(), _stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------
# profile 2 (TNS): decode, and encode behind Encoder(..., allow_profile2=True) (the reference's encoder refuses profile 2)
# ---------------------------------------------------------------------------------------------
P2_DEPTHS = (8, 10, 12, 14, 16, 20, 24)                # ref: fourier/profile2.py:7
P2_LPC = 13                                            # MAX_ORDER + 1 integers per channel (tools/p2tools.py:4)


def _require_int32(t: torch.Tensor, shape: tuple, what: str):
    if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous int32 tensor of shape {list(shape)} (got {t.dtype} {list(t.shape)})")


def p2_golomb_decode_batch(bodies: torch.Tensor, offsets: torch.Tensor, N: int, C: int):
    """The three ``exp_golomb_rice_decode`` calls + ``untrim`` of ``profile2.digital`` (profile2.py:64-76): inflated bodies
    (uint8, frame i at ``offsets[i]:offsets[i+1]``, 8 readable bytes after the last) -> ``(q [n, N, C], tq [n, 27, C],
    lpc [n, 13, C], status [n])``; status 1 = the body's prefix does not fit (decoded as a frame of zeros)."""
    n_frames = _require_ragged(bodies, offsets, "bodies")   # (as p1_golomb_decode_batch: static only)
    q = torch.empty((n_frames, N, C), dtype=torch.int32, device=bodies.device)
    tq = torch.empty((n_frames, P1_BANDS, C), dtype=torch.int32, device=bodies.device)
    lpc = torch.empty((n_frames, P2_LPC, C), dtype=torch.int32, device=bodies.device)
    status = torch.empty(max(n_frames, 1), dtype=torch.int32, device=bodies.device)
    with torch.cuda.device(bodies.device):
        _lib.load().p2_golomb_decode(bodies.data_ptr(), offsets.data_ptr(), n_frames, N, C, q.data_ptr(), tq.data_ptr(),
                                     lpc.data_ptr(), status.data_ptr(), _stream_ptr())
    return q, tq, lpc, status[:n_frames]


def p2_synth_batch(q: torch.Tensor, tq: torch.Tensor, lpc: torch.Tensor, N: int, C: int, bits: int, srate: int) -> torch.Tensor:
    """Dequantisation, TNS synthesis and the threshold ramp of ``profile2.digital`` (profile2.py:69-86): float64 coefficients
    [n_frames, N, C], i.e. a 64-bit little-endian profile-0 payload (``p2_digital_batch`` finishes the frame)."""
    _require_cuda(q, "q"); _require_cuda(tq, "tq"); _require_cuda(lpc, "lpc")
    if bits not in P2_DEPTHS:
        raise ValueError(f"profile 2 depth must be one of {P2_DEPTHS}, got {bits}")
    n_frames = q.shape[0] if q.dim() == 3 else -1
    _require_int32(q, (n_frames, N, C), "q")
    _require_int32(tq, (n_frames, P1_BANDS, C), "tq")
    _require_int32(lpc, (n_frames, P2_LPC, C), "lpc")
    out = torch.empty((n_frames, N, C), dtype=torch.float64, device=q.device)
    with torch.cuda.device(q.device):
        _lib.load().p2_synth(q.data_ptr(), tq.data_ptr(), lpc.data_ptr(), n_frames, N, C, bits, srate, out.data_ptr(), _stream_ptr())
    return out


def p2_analogue_batch(pcm: torch.Tensor, pcm_format: str, n_frames: int, N: int, C: int, bits: int, srate: int,
                      loss_level: float, *, frame_stride: int | None = None, n_valid: int | None = None,
                      raw_be_ints: bool = True) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``profile2.analogue`` up to the Exp-Golomb coder (profile2.py:15-46), batched: frame geometry as ``p1_analogue_batch``;
    ``bits`` one of ``P2_DEPTHS`` (the caller maps any other depth to 16, profile2.py:16).  Returns ``q`` int32 [n_frames, N, C],
    ``tq`` int32 [n_frames, 27, C] and ``lpc`` int32 [n_frames, 13, C] -- the layout ``p2_synth_batch`` reads."""
    if bits not in P2_DEPTHS:
        raise ValueError(f"profile 2 depth must be one of {P2_DEPTHS}, got {bits}")
    if not 1 <= C <= 64:
        raise ValueError(f"profile 2 takes 1 to 64 channels, got {C}")
    code = pcm_dtype_code(pcm_format)
    hop = N if frame_stride is None else frame_stride
    nv = N if n_valid is None else n_valid
    if n_frames < 0 or hop < 0 or not 0 <= nv <= N:
        raise ValueError(f"bad frame geometry: n_frames={n_frames} frame_stride={hop} n_valid={nv} N={N}")
    _require_pcm_span(pcm, n_frames, hop, nv, C, code)
    _require_cuda(pcm, "pcm")
    q = torch.empty((n_frames, N, C), dtype=torch.int32, device=pcm.device)
    tq = torch.empty((n_frames, P1_BANDS, C), dtype=torch.int32, device=pcm.device)
    lpc = torch.empty((n_frames, P2_LPC, C), dtype=torch.int32, device=pcm.device)
    flags = int(raw_be_ints) * _lib.FRAD_RAW_BE_INTS
    with torch.cuda.device(pcm.device):
        _lib.load().p2_analogue(pcm.data_ptr(), code, n_frames, N, C, hop, nv, bits, srate, float(loss_level), flags,
                                q.data_ptr(), tq.data_ptr(), lpc.data_ptr(), _stream_ptr())
    return q, tq, lpc


def p2_golomb_encode_batch(q: torch.Tensor, tq: torch.Tensor, lpc: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The Exp-Golomb-Rice stage of ``profile2.analogue`` (profile2.py:48-52) on the device: ``(bodies uint8 [total], offsets
    int64 [n_frames + 1])``, frame i's pre-deflate body ('>H' len + Golomb(lpc) + '>I' len + Golomb(tq) + Golomb(q)) at
    ``bodies[offsets[i]:offsets[i+1]]``.  Deflate stays on the host."""
    if q.dtype != torch.int32 or q.dim() != 3 or not q.is_contiguous():
        raise TypeError("q must be a contiguous int32 tensor [n_frames, N, C]")
    n_frames, N, C = q.shape
    _require_int32(tq, (n_frames, P1_BANDS, C), "tq")
    _require_int32(lpc, (n_frames, P2_LPC, C), "lpc")
    return _golomb_encode(2, q, tq, lpc)


def p2_digital_batch(q: torch.Tensor, tq: torch.Tensor, lpc: torch.Tensor, N: int, C: int, bits: int, srate: int) -> torch.Tensor:
    """``profile2.digital`` from the decoded integers on: ``p2_synth_batch`` then the inverse DCT of the coefficient plane
    (frad_p0_digital at 64-bit little-endian storage, every compact size) -> float64 PCM [n_frames, N, C]."""
    coeffs = p2_synth_batch(q, tq, lpc, N, C, bits, srate)
    return digital_batch(0, coeffs.view(torch.uint8).reshape(coeffs.shape[0], -1), coeffs.shape[0], N, C, 64, True)


def p1_overlap_add(frames: torch.Tensor, overlap_ratio: int, prev_tail: torch.Tensor | None = None, out_format: str | None = None):
    """The decoder's Hann cross-fade over consecutive decoded frames (decoder.py:28-46).

    ``frames`` float64 [n_frames, N, C]; returns ``(out [n_frames, cut, C], next_tail [N - cut, C])``
    with cut = N*(ratio-1)//ratio; ``prev_tail`` is the previous batch's ``next_tail`` (or None).  ``out_format``: the
    caller's ``from_f64(...).astype(fmt)`` (src/decoder.py:23) applied in the same pass -- ``out`` is then a uint8 tensor
    holding ``[n_frames, cut, C]`` elements of that PCM format (frad_p1_overlap_add_pcm); the tail stays float64."""
    _require_cuda(frames, "frames")
    n_frames, N, C = frames.shape
    cut = N * (overlap_ratio - 1) // overlap_ratio
    nxt = torch.empty((N - cut, C), dtype=torch.float64, device=frames.device)
    if prev_tail is not None:
        _require_cuda(prev_tail, "prev_tail")
        if tuple(prev_tail.shape) != (N - cut, C):
            raise ValueError("prev_tail must be [N - cut, C]")
    pt = prev_tail.data_ptr() if prev_tail is not None else 0
    with torch.cuda.device(frames.device):
        if out_format is not None and out_format not in ("f64le",):
            out = _pcm_out_tensor(out_format, (n_frames, cut, C), frames.device, slack=16)
            _lib.load().p1_overlap_add_pcm(frames.data_ptr(), n_frames, N, C, overlap_ratio, pt, pcm_dtype_code(out_format), out.data_ptr(), nxt.data_ptr(), _stream_ptr())
        else:
            out = torch.empty((n_frames, cut, C), dtype=torch.float64, device=frames.device)
            _lib.load().p1_overlap_add(frames.data_ptr(), n_frames, N, C, overlap_ratio, pt, out.data_ptr(), nxt.data_ptr(), _stream_ptr())
    return out, nxt


def clips_overlap_add(frames: torch.Tensor | None, clip_frame0, N: int, C: int, overlap_ratio: int, tails: torch.Tensor | None = None,
                      tail_off=None, tail_rows=None, out_format: str | None = None, tail_win=None) -> torch.Tensor:
    """``Decoder.overlap`` + ``flush()`` (decoder.py:28-46, 110-114) for many independent clips in one launch, with ragged
    output (frad_clips_overlap_add).

    ``frames`` float64 [n_frames, N, C]: the equal-length decoded frames, clip after clip; ``clip_frame0`` (host integers,
    n_clips + 1, non-decreasing from 0 to n_frames) says which belong to clip j.  ``tails`` flat float64: clip j's last frame of
    another length is ``tail_rows[j]`` rows of C at element offset ``tail_off[j]`` (0 rows: none).  ``overlap_ratio`` 0: no
    fade (cut = N); 2..256: the Hann cross-fade of ``p1_overlap_add`` inside each clip, first frames unfaded, the flush fragment
    appended.  ``tail_win``: see include/frad_hip.h.  Returns ``(out, out_off)``: ``out`` float64 [rows, C], or with
    ``out_format`` a uint8 tensor of that format's bytes as ``p1_overlap_add`` returns them; clip j is rows
    ``out_off[j]:out_off[j+1]`` (numpy int64).  The index arrays are checked here, on the host, before anything is launched."""
    cf = np.ascontiguousarray(clip_frame0, np.int64).reshape(-1)
    n_clips = cf.size - 1
    if n_clips < 0:
        raise ValueError("clip_frame0 needs n_clips + 1 entries")
    if N < 1 or C < 1 or not (overlap_ratio == 0 or 2 <= overlap_ratio <= 256):
        raise ValueError(f"bad geometry: N={N} C={C} overlap_ratio={overlap_ratio}")
    n_frames = int(cf[-1])
    if cf[0] != 0 or (np.diff(cf) < 0).any():
        raise ValueError("clip_frame0 must start at 0 and not decrease")
    if n_frames:
        if frames is None:
            raise ValueError("frames is missing")
        _require_cuda(frames, "frames")
        if frames.dtype != torch.float64 or frames.numel() != n_frames * N * C:
            raise ValueError(f"frames must be float64 [{n_frames}, {N}, {C}]")
    device = frames.device if frames is not None else (tails.device if tails is not None else torch.device("cuda", torch.cuda.current_device()))
    tr = np.zeros(n_clips, np.int32) if tail_rows is None else np.ascontiguousarray(tail_rows, np.int32).reshape(-1)
    to = np.zeros(n_clips, np.int64) if tail_off is None else np.ascontiguousarray(tail_off, np.int64).reshape(-1)
    if tr.size != n_clips or to.size != n_clips:
        raise ValueError("tail_off and tail_rows need one entry per clip")
    cut = N * (overlap_ratio - 1) // overlap_ratio if overlap_ratio else N
    L = N - cut
    if ((tr < 0) | ((tr > 0) & (tr < L))).any():
        raise ValueError(f"a last frame needs at least L = {L} rows")
    has = tr > 0
    if has.any():
        if tails is None:
            raise ValueError("tails is missing")
        _require_cuda(tails, "tails")
        if tails.dtype != torch.float64:
            raise TypeError("tails must be float64")
        if (to[has] < 0).any() or (to[has] + tr[has].astype(np.int64) * C > tails.numel()).any():
            raise ValueError("a last frame lies outside tails")
    m = np.diff(cf)
    rows = m * cut + np.where(has, tr.astype(np.int64), np.where(m > 0, L, 0))
    out_off = np.zeros(n_clips + 1, np.int64)
    np.cumsum(rows, out=out_off[1:])
    total = int(out_off[-1])
    win = None
    if tail_win is not None and L:
        win = np.ascontiguousarray(tail_win, np.float64).reshape(-1)
        if win.size != L:
            raise ValueError(f"tail_win must hold L = {L} weights")
    code = pcm_dtype_code(out_format) if out_format is not None else pcm_dtype_code("f64le")
    if out_format is None:
        out = torch.empty((total, C), dtype=torch.float64, device=device)
    else:
        out = _pcm_out_tensor(out_format, (total, C), device, slack=16)
    if total == 0 or n_clips == 0:
        return out, out_off
    # the four index tables (and the window) in one upload: int64 clip_frame0 | out_off | tail_off | float64 window | int32 tail_rows
    n1 = n_clips + 1
    nw = win.size if win is not None else 0
    table = np.empty(8 * (2 * n1 + n_clips + nw) + 4 * n_clips, np.uint8)
    table[:8 * n1] = cf.view(np.uint8)
    table[8 * n1:16 * n1] = out_off.view(np.uint8)
    table[16 * n1:16 * n1 + 8 * n_clips] = to.view(np.uint8)
    w0 = 16 * n1 + 8 * n_clips
    if nw:
        table[w0:w0 + 8 * nw] = win.view(np.uint8)
    table[w0 + 8 * nw:] = tr.view(np.uint8)
    dev = torch.from_numpy(table).to(device)
    p = dev.data_ptr()
    with torch.cuda.device(device):
        _lib.load().clips_overlap_add(frames.data_ptr() if n_frames else 0, p, n_clips, N, C, overlap_ratio,
                                      tails.data_ptr() if tails is not None else 0, p + 16 * n1, p + w0 + 8 * nw, p + w0 if nw else 0,
                                      code, out.data_ptr(), p + 8 * n1, total, _stream_ptr())
    return out, out_off


def _require_device_tensor(t, what: str):
    """``_require_cuda`` for an operator whose every failed host check is a ValueError"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous tensor in MI355X device memory")


def clips_carry_add(frames: torch.Tensor | None, clip_frame0, N: int, C: int, overlap_ratio: int, prev=None, nxt=None,
                    out_format: str | None = None, out: torch.Tensor | None = None):
    """``p1_overlap_add`` for many live streams in one launch (frad_clips_carry_add): clip j is the next ``m_j`` whole frames of a
    stream that is still arriving, cross-faded from the fragment it carried in to the fragment it carries out.

    ``frames`` float64 [n, N, C]; ``clip_frame0`` (host integers, n_clips + 1, non-decreasing, inside ``frames``) says which
    belong to clip j.  ``prev`` / ``nxt``: None, or per clip None or a float64 device tensor of ``L * C`` elements -- the
    fragment read, and the buffer that takes rows ``[cut, N)`` of the clip's last frame (left alone when ``m_j == 0``); a clip's
    two must differ.  With ``overlap_ratio`` 0 nothing is faded or carried.  Returns ``(out, out_off)``: clip j is rows
    ``out_off[j]:out_off[j+1]`` (``m_j * cut`` of them) of ``out``, float64 [rows, C] or with ``out_format`` that format's
    bytes as ``p1_overlap_add`` returns them; ``out``, when given, is written from its start and must hold them.  Every table
    is checked here, on the host, before anything is launched."""
    cf = np.ascontiguousarray(clip_frame0, np.int64).reshape(-1)
    n_clips = cf.size - 1
    if n_clips < 0:
        raise ValueError("clip_frame0 needs n_clips + 1 entries")
    if N < 1 or C < 1 or not (overlap_ratio == 0 or 2 <= overlap_ratio <= 256):
        raise ValueError(f"bad geometry: N={N} C={C} overlap_ratio={overlap_ratio}")
    cut = N * (overlap_ratio - 1) // overlap_ratio if overlap_ratio else N
    L = N - cut
    if cut < 1:
        raise ValueError(f"bad geometry: N={N} keeps no row at overlap_ratio={overlap_ratio}")
    if cf[0] < 0 or (np.diff(cf) < 0).any():
        raise ValueError("clip_frame0 must not be negative and must not decrease")
    m = np.diff(cf)
    if cf[-1] > cf[0]:
        if frames is None:
            raise ValueError("frames is missing")
        _require_device_tensor(frames, "frames")
        if frames.dtype != torch.float64 or frames.numel() % (N * C):
            raise ValueError(f"frames must be float64 [n, {N}, {C}]")
        if cf[-1] > frames.numel() // (N * C):
            raise ValueError("a clip's frames lie outside frames")
    device = frames.device if frames is not None else (out.device if out is not None else torch.device("cuda", torch.cuda.current_device()))
    ptrs = np.zeros((2, max(n_clips, 1)), np.uint64)
    for row, (name, table) in enumerate((("prev", prev), ("nxt", nxt))):
        if table is None or not L:
            continue
        if len(table) != n_clips:
            raise ValueError(f"{name} needs one entry per clip")
        for j, t in enumerate(table):
            if t is None:
                continue
            _require_device_tensor(t, f"{name}[{j}]")
            if t.dtype != torch.float64 or t.numel() != L * C or t.device != device:
                raise ValueError(f"{name}[{j}] must be float64 [{L}, {C}] on {device}")
            if t.data_ptr() % 8:
                raise ValueError(f"{name}[{j}] must be 8-byte aligned")
            ptrs[row, j] = t.data_ptr()
    pp, nn = ptrs[0, :n_clips], ptrs[1, :n_clips]
    if ((pp != 0) & (pp == nn)).any():
        raise ValueError("a clip's prev and nxt must be different buffers")
    rd, wr = np.sort(pp[pp != 0]), nn[(nn != 0) & (m > 0)]
    if rd.size and wr.size:
        # no fragment written may be one that is read: the launch reads and writes them in no order
        span = np.uint64(L * C * 8)
        at = np.searchsorted(rd, wr + span, side="left")       # the last read that starts below the end of the write ...
        if ((at > 0) & (rd[np.maximum(at, 1) - 1] + span > wr)).any():             # ... ends above its start
            raise ValueError("a nxt buffer overlaps a prev buffer")
    out_off = np.zeros(n_clips + 1, np.int64)
    np.cumsum(m * cut, out=out_off[1:])
    total = int(out_off[-1])
    code = pcm_dtype_code(out_format) if out_format is not None else pcm_dtype_code("f64le")
    if out is None:
        out = torch.empty((total, C), dtype=torch.float64, device=device) if out_format is None else \
            _pcm_out_tensor(out_format, (total, C), device, slack=16)
    else:
        _require_device_tensor(out, "out")
        if out.dtype != (torch.float64 if out_format is None else torch.uint8):
            raise ValueError("out must be float64, or with out_format the uint8 bytes of that format")
        if out.numel() * out.element_size() < total * C * itemsize_of(code):
            raise ValueError(f"out is too small for {total} sample-frames")
    if total == 0 or n_clips == 0:
        return out, out_off
    _require_frame_count(n_clips, "clips")
    # the four tables in one upload: int64 clip_frame0 | out_off, then the prev and the nxt pointers
    n1 = n_clips + 1
    table = np.concatenate([cf.view(np.uint8), out_off.view(np.uint8), ptrs[0, :n_clips].view(np.uint8), ptrs[1, :n_clips].view(np.uint8)])
    dev = torch.from_numpy(table).to(device)
    p = dev.data_ptr()
    with torch.cuda.device(device):
        _lib.load().clips_carry_add(frames.data_ptr(), p, n_clips, N, C, overlap_ratio, p + 16 * n1 if L else 0,
                                    p + 16 * n1 + 8 * n_clips if L else 0, code, _lib.FRAD_RAW_BE_INTS, out.data_ptr(), p + 8 * n1, total,
                                    _stream_ptr())
    return out, out_off


def clips_window_add(frames: torch.Tensor | None, clip_f0, clip_m, N: int, C: int, overlap_ratio: int, tails: torch.Tensor | None = None,
                     tail_off=None, tail_rows=None, skip=None, valid=None, out_format: str | None = None, tail_win=None, span=None,
                     dst_row=None, out: torch.Tensor | None = None):
    """Rows ``[skip[j], skip[j] + valid[j])`` of the timeline ``clips_overlap_add`` writes for clip j, for many clips in one launch
    (frad_clips_window_add); bit for bit the slice of its output.

    ``frames`` float64 [n_frames, N, C]; clip j is frames ``clip_f0[j] : clip_f0[j] + clip_m[j]`` and the last frame
    ``tail_rows[j]`` rows at element ``tail_off[j]`` of ``tails`` -- clips may share frames and tails.  ``skip`` defaults to 0,
    ``valid`` to the rest of the timeline.  Clip j's span is ``span[j]`` sample-frames (default ``valid[j]``), its rows from
    ``valid[j]`` on are ``out_format``'s silence.  Without ``dst_row`` the spans follow each other in a fresh ``out``; with
    ``dst_row`` (and ``out``, a contiguous device tensor of float64 or of ``out_format``'s bytes) span j starts at sample-frame
    ``dst_row[j]`` of ``out`` and nothing else of ``out`` is written.  Returns ``(out, out_off)``, span j at rows
    ``out_off[j]:out_off[j+1]`` of a fresh ``out``.  Every table is checked here, on the host, before anything is launched."""
    f0 = np.ascontiguousarray(clip_f0, np.int64).reshape(-1)
    m = np.ascontiguousarray(clip_m, np.int32).reshape(-1)
    n_clips = f0.size
    if N < 1 or C < 1 or not (overlap_ratio == 0 or 2 <= overlap_ratio <= 256):
        raise ValueError(f"bad geometry: N={N} C={C} overlap_ratio={overlap_ratio}")
    tr = np.zeros(n_clips, np.int32) if tail_rows is None else np.ascontiguousarray(tail_rows, np.int32).reshape(-1)
    to = np.zeros(n_clips, np.int64) if tail_off is None else np.ascontiguousarray(tail_off, np.int64).reshape(-1)
    sk = np.zeros(n_clips, np.int64) if skip is None else np.ascontiguousarray(skip, np.int64).reshape(-1)
    if m.size != n_clips or tr.size != n_clips or to.size != n_clips or sk.size != n_clips:
        raise ValueError("clip_m, tail_off, tail_rows and skip need one entry per clip")
    cut = N * (overlap_ratio - 1) // overlap_ratio if overlap_ratio else N
    L = N - cut
    used = m > 0
    if (m < 0).any() or (f0[used] < 0).any():
        raise ValueError("clip_f0 and clip_m must not be negative")
    if used.any():
        if frames is None:
            raise ValueError("frames is missing")
        _require_cuda(frames, "frames")
        if frames.dtype != torch.float64 or frames.numel() % (N * C):
            raise ValueError(f"frames must be float64 [n, {N}, {C}]")
        if (f0[used] > frames.numel() // (N * C) - m[used].astype(np.int64)).any():
            raise ValueError("a clip's frames lie outside frames")
    if ((tr < 0) | ((tr > 0) & (tr < L))).any():
        raise ValueError(f"a last frame needs at least L = {L} rows")
    has = tr > 0
    if has.any():
        if tails is None:
            raise ValueError("tails is missing")
        _require_cuda(tails, "tails")
        if tails.dtype != torch.float64:
            raise TypeError("tails must be float64")
        if (to[has] < 0).any() or (to[has] > tails.numel() - tr[has].astype(np.int64) * C).any():
            raise ValueError("a last frame lies outside tails")
    timeline = m.astype(np.int64) * cut + np.where(has, tr.astype(np.int64), np.where(used, L, 0))
    if (sk < 0).any() or (sk > timeline).any():
        raise ValueError("skip lies outside the clip's timeline")
    va = (timeline - sk).astype(np.int32) if valid is None else np.ascontiguousarray(valid, np.int32).reshape(-1)
    if va.size != n_clips or (va < 0).any() or (va.astype(np.int64) > timeline - sk).any():
        raise ValueError("skip + valid must end inside the clip's timeline")
    sp = va.astype(np.int64) if span is None else np.ascontiguousarray(span, np.int64).reshape(-1)
    if sp.size != n_clips or (sp < va).any():
        raise ValueError("a span must hold its clip's valid rows")
    out_off = np.zeros(n_clips + 1, np.int64)
    np.cumsum(sp, out=out_off[1:])
    total = int(out_off[-1])
    win = None
    if tail_win is not None and L:
        win = np.ascontiguousarray(tail_win, np.float64).reshape(-1)
        if win.size != L:
            raise ValueError(f"tail_win must hold L = {L} weights")
    code = pcm_dtype_code(out_format) if out_format is not None else pcm_dtype_code("f64le")
    device = frames.device if frames is not None else (tails.device if tails is not None else out.device if out is not None
                                                       else torch.device("cuda", torch.cuda.current_device()))
    dst = None
    if dst_row is None:
        if out is not None:
            raise ValueError("out goes with dst_row")
        out = torch.empty((total, C), dtype=torch.float64, device=device) if out_format is None else \
            _pcm_out_tensor(out_format, (total, C), device, slack=16)
    else:
        dst = np.ascontiguousarray(dst_row, np.int64).reshape(-1)
        if out is None or dst.size != n_clips:
            raise ValueError("dst_row needs out and one entry per clip")
        _require_cuda(out, "out")
        if out.dtype != (torch.float64 if out_format is None else torch.uint8):
            raise TypeError("out must be float64, or with out_format the uint8 bytes of that format")
        have = out.numel() * out.element_size() // (C * itemsize_of(code))
        if (dst < 0).any() or (dst > have - sp).any():
            raise ValueError(f"a span lies outside out ({have} sample-frames)")
        order = np.argsort(dst, kind="stable")
        order = order[sp[order] > 0]
        if (dst[order][:-1] + sp[order][:-1] > dst[order][1:]).any():
            raise ValueError("the spans overlap")
    if total == 0 or n_clips == 0:
        return out, out_off
    _require_frame_count(n_clips, "clips")
    # every table (and the window) in one upload: int64 clip_f0 | out_off | tail_off | skip | dst_row, float64 window, int32 clip_m | tail_rows | valid
    wide = [f0, out_off, to, sk] + ([dst] if dst is not None else []) + ([win] if win is not None else [])
    table = np.concatenate([a.view(np.uint8) for a in wide + [m, tr, va]])
    dev = torch.from_numpy(table).to(device)
    p, at, ptr = dev.data_ptr(), 0, []
    for a in wide + [m, tr, va]:
        ptr.append(p + at)
        at += a.nbytes
    p_f0, p_off, p_to, p_sk = ptr[:4]
    p_dst = ptr[4] if dst is not None else 0
    p_win = ptr[len(wide) - 1] if win is not None else 0
    p_m, p_tr, p_va = ptr[-3:]
    with torch.cuda.device(device):
        _lib.load().clips_window_add(frames.data_ptr() if frames is not None else 0, p_f0, p_m, n_clips, N, C, overlap_ratio,
                                     tails.data_ptr() if tails is not None else 0, p_to, p_tr, p_win, p_sk, p_va, p_dst, code,
                                     _lib.FRAD_RAW_BE_INTS, out.data_ptr(), p_off, total, _stream_ptr())
    return out, out_off


def clips_resample(src: torch.Tensor | None, src_off, src_row0, src_rows, C: int, up: int, down: int, taps: torch.Tensor, out_row0,
                   valid, out_format: str | None = None, span=None, dst_row=None, out: torch.Tensor | None = None):
    """Polyphase resampling by ``up / down`` of many ragged float64 spans in one launch (frad_clips_resample), converted and
    written as ``clips_window_add`` writes its windows.

    ``src`` flat float64: clip j's source rows are ``src_rows[j]`` rows of ``C`` at element ``src_off[j]``, rows ``src_row0[j] ..``
    of the stream's timeline; rows outside count as zero; spans may overlap.  ``taps``: the device copy of
    ``window.resample_taps(up, down)``.  Rows ``out_row0[j] : out_row0[j] + valid[j]`` of the resampled stream are written to
    clip j's span of ``span[j]`` sample-frames (default ``valid[j]``), the rest of the span is ``out_format``'s silence; ``dst_row``
    and ``out`` as for ``clips_window_add``.  Returns ``(out, out_off)``.  Every table is checked here, on the host, before
    anything is launched."""
    so = np.ascontiguousarray(src_off, np.int64).reshape(-1)
    s0 = np.ascontiguousarray(src_row0, np.int64).reshape(-1)
    sr = np.ascontiguousarray(src_rows, np.int32).reshape(-1)
    o0 = np.ascontiguousarray(out_row0, np.int64).reshape(-1)
    va = np.ascontiguousarray(valid, np.int32).reshape(-1)
    n_clips = so.size
    if C < 1 or up < 1 or down < 1:
        raise ValueError(f"bad geometry: C={C} up={up} down={down}")
    if s0.size != n_clips or sr.size != n_clips or o0.size != n_clips or va.size != n_clips:
        raise ValueError("src_off, src_row0, src_rows, out_row0 and valid need one entry per clip")
    half = 10 * max(up, down)
    _require_cuda(taps, "taps")
    if taps.dtype != torch.float64 or taps.numel() != 2 * half + 1:
        raise ValueError(f"taps must be the {2 * half + 1} float64 taps of {up}/{down}")
    if (sr < 0).any() or (s0 < 0).any() or (o0 < 0).any() or (va < 0).any():
        raise ValueError("src_row0, src_rows, out_row0 and valid must not be negative")
    used = sr > 0
    if used.any():
        if src is None:
            raise ValueError("src is missing")
        _require_cuda(src, "src")
        if src.dtype != torch.float64:
            raise TypeError("src must be float64")
        if (so[used] < 0).any() or (so[used] > src.numel() - sr[used].astype(np.int64) * C).any():
            raise ValueError("a clip's source rows lie outside src")
    sp = va.astype(np.int64) if span is None else np.ascontiguousarray(span, np.int64).reshape(-1)
    if sp.size != n_clips or (sp < va).any():
        raise ValueError("a span must hold its clip's valid rows")
    out_off = np.zeros(n_clips + 1, np.int64)
    np.cumsum(sp, out=out_off[1:])
    total = int(out_off[-1])
    code = pcm_dtype_code(out_format) if out_format is not None else pcm_dtype_code("f64le")
    device = taps.device
    dst = None
    if dst_row is None:
        if out is not None:
            raise ValueError("out goes with dst_row")
        out = torch.empty((total, C), dtype=torch.float64, device=device) if out_format is None else \
            _pcm_out_tensor(out_format, (total, C), device, slack=16)
    else:
        dst = np.ascontiguousarray(dst_row, np.int64).reshape(-1)
        if out is None or dst.size != n_clips:
            raise ValueError("dst_row needs out and one entry per clip")
        _require_cuda(out, "out")
        if out.dtype != (torch.float64 if out_format is None else torch.uint8):
            raise TypeError("out must be float64, or with out_format the uint8 bytes of that format")
        have = out.numel() * out.element_size() // (C * itemsize_of(code))
        if (dst < 0).any() or (dst > have - sp).any():
            raise ValueError(f"a span lies outside out ({have} sample-frames)")
        order = np.argsort(dst, kind="stable")
        order = order[sp[order] > 0]
        if (dst[order][:-1] + sp[order][:-1] > dst[order][1:]).any():
            raise ValueError("the spans overlap")
    if total == 0 or n_clips == 0:
        return out, out_off
    _require_frame_count(n_clips, "clips")
    # every table in one upload: int64 src_off | src_row0 | out_row0 | out_off | dst_row, int32 src_rows | valid
    wide = [so, s0, o0, out_off] + ([dst] if dst is not None else [])
    table = np.concatenate([a.view(np.uint8) for a in wide + [sr, va]])
    dev = torch.from_numpy(table).to(device)
    p, at, ptr = dev.data_ptr(), 0, []
    for a in wide + [sr, va]:
        ptr.append(p + at)
        at += a.nbytes
    with torch.cuda.device(device):
        _lib.load().clips_resample(src.data_ptr() if used.any() else 0, ptr[0], ptr[1], ptr[-2], n_clips, C, up, down, taps.data_ptr(), half,
                                   ptr[2], ptr[-1], ptr[4] if dst is not None else 0, code, _lib.FRAD_RAW_BE_INTS, out.data_ptr(), ptr[3],
                                   total, _stream_ptr())
    return out, out_off


def clips_remix(srcs, mats, C_out: int, valid=None, out_format: str | None = None, span=None, dst_row=None,
                out: torch.Tensor | None = None):
    """A channel mix of many ragged float64 spans in one launch (frad_clips_remix), converted and written as ``clips_window_add``
    writes its windows.

    ``srcs``: a list of float64 device tensors ``[rows_j, C_in_j]``, one per clip -- the channel counts may differ; an entry may
    be None where ``valid[j]`` is 0.  ``mats``: the clips' matrices ``[C_out, C_in_j]`` (host, float64, finite), as a list with one
    per clip or a dict with one per distinct ``C_in``.  Output row r < ``valid[j]`` (default ``rows_j``) of clip j is ``mats[j] @
    srcs[j][r]`` in the entry point's arithmetic (include/frad_hip.h: zero weights are skipped, a multiply and an add per term);
    the rest of the span of ``span[j]`` sample-frames (default ``valid[j]``) is ``out_format``'s silence; ``dst_row`` and ``out`` as
    for ``clips_window_add``.  Returns ``(out, out_off)``.  Everything is checked here, on the host, before anything is launched,
    and the tensors' addresses are taken only here."""
    srcs = list(srcs)
    n_clips = len(srcs)
    if C_out < 1:
        raise ValueError(f"bad geometry: C_out={C_out}")
    per_cin = isinstance(mats, dict)
    if not per_cin:
        mats = list(mats)
        if len(mats) != n_clips:
            raise ValueError("mats needs one matrix per clip (or a dict with one per channel count)")
    device = next((s.device for s in srcs if s is not None), None)
    rows, ch, addr = np.zeros(n_clips, np.int64), np.ones(n_clips, np.int32), np.zeros(n_clips, np.int64)
    for j, s in enumerate(srcs):
        if s is None:
            continue
        _require_cuda(s, f"srcs[{j}]")
        if s.dtype != torch.float64 or s.dim() != 2 or s.shape[1] < 1:
            raise ValueError(f"srcs[{j}] must be float64 [rows, channels]")
        if s.device != device:
            raise ValueError("the clips must live on one device")
        rows[j], ch[j] = s.shape
        addr[j] = s.data_ptr() if s.shape[0] else 0
        if addr[j] % 8:
            raise ValueError(f"srcs[{j}] is not 8-byte aligned")
    va = rows.astype(np.int32) if valid is None else np.ascontiguousarray(valid, np.int32).reshape(-1)
    if va.size != n_clips or (va < 0).any() or (va > rows).any():
        raise ValueError("valid needs one entry per clip, 0 <= valid[j] <= the clip's rows")
    # ---- the matrices: each distinct one placed once
    placed, flat, at = {}, [], 0
    mat_off = np.zeros(n_clips, np.int64)
    for j, s in enumerate(srcs):
        if s is None:
            continue                                           # (no row of this clip is read: neither is its matrix)
        key = int(ch[j]) if per_cin else id(mats[j])
        if key not in placed:
            if per_cin and key not in mats:
                raise ValueError(f"no matrix for the clips of {key} channels")
            m = np.asarray(mats[key] if per_cin else mats[j], np.float64)
            if m.ndim != 2 or m.shape != (C_out, int(ch[j])):
                raise ValueError(f"clip {j} needs a matrix [{C_out}, {int(ch[j])}] (got {list(m.shape)})")
            if not np.isfinite(m).all():
                raise ValueError(f"the matrix of clip {j} is not finite")
            placed[key] = (at, m.shape)
            flat.append(np.ascontiguousarray(m).reshape(-1))
            at += m.size
        elif placed[key][1] != (C_out, int(ch[j])):
            raise ValueError(f"clip {j} needs a matrix [{C_out}, {int(ch[j])}] (got {list(placed[key][1])})")
        mat_off[j] = placed[key][0]
    sp = va.astype(np.int64) if span is None else np.ascontiguousarray(span, np.int64).reshape(-1)
    if sp.size != n_clips or (sp < va).any():
        raise ValueError("a span must hold its clip's valid rows")
    out_off = np.zeros(n_clips + 1, np.int64)
    np.cumsum(sp, out=out_off[1:])
    total = int(out_off[-1])
    code = pcm_dtype_code(out_format) if out_format is not None else pcm_dtype_code("f64le")
    if device is None:
        device = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
    dst = None
    if dst_row is None:
        if out is not None:
            raise ValueError("out goes with dst_row")
        out = torch.empty((total, C_out), dtype=torch.float64, device=device) if out_format is None else \
            _pcm_out_tensor(out_format, (total, C_out), device, slack=16)
    else:
        dst = np.ascontiguousarray(dst_row, np.int64).reshape(-1)
        if out is None or dst.size != n_clips:
            raise ValueError("dst_row needs out and one entry per clip")
        _require_cuda(out, "out")
        if out.dtype != (torch.float64 if out_format is None else torch.uint8):
            raise TypeError("out must be float64, or with out_format the uint8 bytes of that format")
        if out.device != device:
            raise ValueError("out must live on the clips' device")
        have = out.numel() * out.element_size() // (C_out * itemsize_of(code))
        if (dst < 0).any() or (dst > have - sp).any():
            raise ValueError(f"a span lies outside out ({have} sample-frames)")
        order = np.argsort(dst, kind="stable")
        order = order[sp[order] > 0]
        if (dst[order][:-1] + sp[order][:-1] > dst[order][1:]).any():
            raise ValueError("the spans overlap")
    if total == 0 or n_clips == 0:
        return out, out_off
    _require_frame_count(n_clips, "clips")
    # every table in one upload: int64 src_ptr | mat_off | out_off | dst_row, float64 matrices, int32 src_ch | valid
    weights = np.concatenate(flat) if flat else np.zeros(1)
    parts = [addr, mat_off, out_off] + ([dst] if dst is not None else []) + [weights, ch, va]
    table = np.concatenate([a.view(np.uint8) for a in parts])
    dev = torch.from_numpy(table).to(device)
    p, at, ptr = dev.data_ptr(), 0, []
    for a in parts:
        ptr.append(p + at)
        at += a.nbytes
    with torch.cuda.device(device):
        _lib.load().clips_remix(ptr[0], ptr[-2], ptr[-3], ptr[1], n_clips, C_out, ptr[-1], ptr[3] if dst is not None else 0, code,
                                _lib.FRAD_RAW_BE_INTS, out.data_ptr(), ptr[2], total, _stream_ptr())
    return out, out_off


def spectrum_tables_check(tb) -> None:
    """The host checks of a ``spectral.SpecTables`` for ``clips_spectrum`` (ValueError): geometry, window, bands, logarithm."""
    n_fft = tb.n_fft
    if n_fft not in (128, 256, 512, 1024, 2048, 4096):
        raise ValueError(f"n_fft is a power of two from 128 to 4096 (got {n_fft})")
    if tb.hop < 1 or tb.power not in (1, 2):
        raise ValueError(f"bad geometry: hop={tb.hop}, power={tb.power}")
    w = np.asarray(tb.window)
    if w.dtype != np.float64 or w.shape != (n_fft,) or not np.isfinite(w).all():
        raise ValueError(f"the window must be {n_fft} finite float64 weights (win_length <= n_fft, zero-padded)")
    if np.dtype(tb.dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"the output is float32 or float64 (got {tb.dtype})")
    if tb.band_lo is not None:
        lo, ln, off, bw = (np.asarray(a) for a in (tb.band_lo, tb.band_len, tb.band_off, tb.band_w))
        if lo.dtype != np.int32 or ln.dtype != np.int32 or off.dtype != np.int64 or bw.dtype != np.float64 or bw.ndim != 1:
            raise ValueError("the bands are int32 band_lo / band_len, int64 band_off and float64 weights")
        if not (lo.shape == ln.shape == off.shape) or lo.ndim != 1 or lo.size < 1:
            raise ValueError("band_lo, band_len and band_off need one entry per output bin")
        if (lo < 0).any() or (ln < 0).any() or (lo.astype(np.int64) + ln > n_fft // 2 + 1).any():
            raise ValueError(f"a band leaves the bins [0, {n_fft // 2}]")
        if (off < 0).any() or (off + ln > bw.size).any():
            raise ValueError("a band leaves the weight array")
        if not np.isfinite(bw).all():
            raise ValueError("the filterbank is not finite")
    if tb.log_scale:
        if not (np.isfinite(tb.log_scale) and np.isfinite(tb.floor) and tb.floor > 0 and np.isfinite(tb.floor_log)):
            raise ValueError(f"a logarithm needs a finite floor > 0 (got {tb.floor})")


def spectrum_tables_upload(tb, device) -> dict:
    """the window and the bands of a checked ``SpecTables`` in one upload -> what ``clips_spectrum(dev_tables=)`` takes"""
    has = tb.band_lo is not None
    parts = [np.ascontiguousarray(tb.window, np.float64)]
    if has:
        parts += [np.ascontiguousarray(tb.band_w, np.float64), np.ascontiguousarray(tb.band_off, np.int64),
                  np.ascontiguousarray(tb.band_lo, np.int32), np.ascontiguousarray(tb.band_len, np.int32)]
    dev = torch.from_numpy(np.concatenate([a.view(np.uint8) for a in parts] + [np.zeros(8, np.uint8)])).to(device)
    ptr, at = [], dev.data_ptr()
    for a in parts:
        ptr.append(at)
        at += a.nbytes
    return dict(keep=dev, window=ptr[0], band_w=ptr[1] if has else 0, band_off=ptr[2] if has else 0, band_lo=ptr[3] if has else 0,
                band_len=ptr[4] if has else 0, n_bands=len(tb.band_lo) if has else 0, n_weights=len(tb.band_w) if has else 0)


def clips_spectrum(srcs, valid, tb, K: int, frame_off, out: torch.Tensor | None = None, dev_tables: dict | None = None) -> torch.Tensor:
    """Spectrograms of many ragged float64 windows in one launch (frad_clips_spectrum; include/frad_hip.h).

    ``srcs``: a list of float64 device tensors ``[rows_j, K]``, one per clip (None where ``valid[j]`` is 0); ``valid[j] <=
    rows_j`` (default ``rows_j``): the rows that count, every other row is zero.  ``tb``: a ``spectral.SpecTables`` (host):
    geometry, window, bands, logarithm, output type.  ``frame_off`` int64 ``[n_clips + 1]``, ascending: clip j owns the frames
    ``frame_off[j] : frame_off[j + 1]`` of the output, the first of them its frame 0 -- ``j * F`` for a dense batch.  ``out``:
    ``[frame_off[-1], K, n_bins]`` of the tables' dtype (allocated when None).  ``dev_tables``: ``spectrum_tables_upload(tb,
    device)`` kept by the caller, so that a spec's tables are uploaded once.  Everything is checked here, on the host, before
    anything is launched, and the tensors' addresses are taken only here."""
    srcs = list(srcs)
    n_clips = len(srcs)
    if K < 1:
        raise ValueError(f"bad geometry: K={K}")
    spectrum_tables_check(tb)
    device = next((s.device for s in srcs if s is not None), None)
    rows, addr = np.zeros(n_clips, np.int64), np.zeros(n_clips, np.int64)
    for j, s in enumerate(srcs):
        if s is None:
            continue
        _require_cuda(s, f"srcs[{j}]")
        if s.dtype != torch.float64 or s.dim() != 2 or s.shape[1] != K:
            raise ValueError(f"srcs[{j}] must be float64 [rows, {K}]")
        if s.device != device:
            raise ValueError("the clips must live on one device")
        rows[j] = s.shape[0]
        addr[j] = s.data_ptr() if s.shape[0] else 0
        if addr[j] % 8:
            raise ValueError(f"srcs[{j}] is not 8-byte aligned")
    va = rows.astype(np.int32) if valid is None else np.ascontiguousarray(valid, np.int32).reshape(-1)
    if va.size != n_clips or (va < 0).any() or (va > rows).any():
        raise ValueError("valid needs one entry per clip, 0 <= valid[j] <= the clip's rows")
    off = np.ascontiguousarray(frame_off, np.int64).reshape(-1)
    if off.size != n_clips + 1 or off[0] != 0 or (np.diff(off) < 0).any():
        raise ValueError("frame_off needs n_clips + 1 ascending entries from 0")
    total = int(off[-1])
    tdt = torch.float32 if np.dtype(tb.dtype) == np.dtype(np.float32) else torch.float64
    if device is None:
        device = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = torch.empty((total, K, tb.n_bins), dtype=tdt, device=device)
    else:
        _require_cuda(out, "out")
        if out.dtype != tdt or out.numel() != total * K * tb.n_bins or out.device != device:
            raise ValueError(f"out must be {total} * {K} * {tb.n_bins} values of {tdt} on the clips' device")
    if total == 0 or n_clips == 0:
        return out
    _require_frame_count(n_clips, "clips")
    dt = dev_tables if dev_tables is not None else spectrum_tables_upload(tb, device)
    parts = [addr, off, va]                                    # int64 src_ptr | frame_off, int32 valid: one upload
    dev = torch.from_numpy(np.concatenate([a.view(np.uint8) for a in parts])).to(device)
    p = dev.data_ptr()
    code = pcm_dtype_code("f32le" if tdt == torch.float32 else "f64le")
    with torch.cuda.device(device):
        _lib.load().clips_spectrum(p, p + addr.nbytes + off.nbytes, n_clips, K, p + addr.nbytes, total, tb.n_fft, tb.hop, int(tb.center),
                                   dt["window"], tb.power, dt["n_bands"], dt["band_lo"], dt["band_len"], dt["band_off"], dt["band_w"],
                                   dt["n_weights"], tb.log_scale, tb.floor, tb.floor_log, code, out.data_ptr(), _stream_ptr())
    return out


def clips_frame_cut(src: torch.Tensor, row_src, row_valid, row_len: int, step: int) -> torch.Tensor:
    """The Encoder's frame cut (encoder.py:72-93) for the frames of many clips in one launch (frad_clips_frame_cut).

    ``src`` uint8 [bytes]: the clips' raw interleaved PCM back to back, ``step`` = itemsize * channels bytes per sample-frame.
    Row r of the result is ``row_valid[r]`` sample-frames from sample-frame ``row_src[r]`` of ``src`` on, then zero bytes up to
    ``row_len`` sample-frames (``row_src`` / ``row_valid``: host integers, one per row; rows may overlap).  Returns uint8
    [n_rows, row_len * step], the contiguous block the ``*_analogue_batch`` operators read with ``frame_stride = row_len``.
    The two tables are checked here, on the host, before anything is uploaded or launched."""
    rs = np.ascontiguousarray(row_src, np.int64).reshape(-1)
    rv = np.ascontiguousarray(row_valid, np.int32).reshape(-1)
    if row_len < 1 or step < 1:
        raise ValueError(f"bad geometry: row_len={row_len} step={step}")
    if rs.size != rv.size:
        raise ValueError("row_src and row_valid need one entry per row")
    _require_cuda(src, "src")
    if src.dtype != torch.uint8 or src.dim() != 1:
        raise ValueError(f"src must be a 1-D uint8 tensor (got {src.dtype} {list(src.shape)})")
    n_rows = rs.size
    _require_frame_count(n_rows, "rows")
    have = src.numel() // step
    if ((rv < 0) | (rv > row_len)).any():
        raise ValueError(f"row_valid must lie in [0, {row_len}]")
    if ((rs < 0) | (rs > have - rv.astype(np.int64))).any():                    # (not rs + rv > have: that sum can wrap)
        raise ValueError(f"a row reads outside src ({have} sample-frames)")
    out = torch.empty((n_rows, row_len * step), dtype=torch.uint8, device=src.device)
    if n_rows == 0:
        return out
    table = np.empty(12 * n_rows, np.uint8)                    # int64 row_src | int32 row_valid: one upload
    table[:8 * n_rows] = rs.view(np.uint8)
    table[8 * n_rows:] = rv.view(np.uint8)
    dev = torch.from_numpy(table).to(src.device)
    base = src.data_ptr() if src.numel() else out.data_ptr()   # (every row all padding: nothing is read)
    with torch.cuda.device(src.device):
        _lib.load().clips_frame_cut(base, dev.data_ptr(), dev.data_ptr() + 8 * n_rows, n_rows, row_len, step, out.data_ptr(), _stream_ptr())
    return out


def clips_carry_cut(carry, src: torch.Tensor, src_off, row_clip, row_at, row_len: int, step: int, next_at=None, nxt=None) -> torch.Tensor:
    """``clips_frame_cut`` for clips that are pieces of live streams, and their remainders, in one launch (frad_clips_carry_cut).

    Clip j's sample-frames are ``carry[j]`` (None, or a 1-D uint8 device tensor of whole sample-frames: what the stream carried
    over) followed by sample-frames ``src_off[j]:src_off[j + 1]`` of ``src`` (1-D uint8: the chunks that just arrived, joined);
    ``step`` = itemsize * channels bytes per sample-frame.  Row r of the result is ``row_len`` sample-frames of clip
    ``row_clip[r]`` from its sample-frame ``row_at[r]`` on -- in the carry, in the chunk or across the seam.  ``nxt``: None, or per
    clip None or a 1-D uint8 device tensor that takes the clip's sample-frames from ``next_at[j]`` to its end, exactly that
    long; it must not overlap ``src`` or any carry.  Returns uint8 [n_rows, row_len * step], the contiguous block the
    ``*_analogue_batch`` operators read with ``frame_stride = row_len``.  Every table is host integers and is checked here,
    before anything is uploaded or launched."""
    if row_len < 1 or step < 1:
        raise ValueError(f"bad geometry: row_len={row_len} step={step}")
    so = np.ascontiguousarray(src_off, np.int64).reshape(-1)
    n_clips = so.size - 1
    if n_clips < 0 or len(carry) != n_clips:
        raise ValueError("src_off needs n_clips + 1 entries and carry one per clip")
    rc = np.ascontiguousarray(row_clip, np.int32).reshape(-1)
    ra = np.ascontiguousarray(row_at, np.int64).reshape(-1)
    n_rows = rc.size
    if ra.size != n_rows:
        raise ValueError("row_clip and row_at need one entry per row")
    _require_frame_count(n_rows, "rows")
    _require_frame_count(n_clips, "clips")
    if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8 or src.dim() != 1:
        raise ValueError("src must be a 1-D uint8 tensor")
    if so[0] < 0 or (np.diff(so) < 0).any() or so[-1] > src.numel() // step:
        raise ValueError(f"src_off must not decrease and must stay inside src ({src.numel() // step} sample-frames)")
    clen = np.zeros(max(n_clips, 1), np.int32)
    ptrs = np.zeros((2, max(n_clips, 1)), np.uint64)
    for j, c in enumerate(carry):
        if c is None:
            continue
        if not isinstance(c, torch.Tensor) or c.dtype != torch.uint8 or c.dim() != 1 or c.numel() % step:
            raise ValueError(f"carry[{j}] must be a 1-D uint8 tensor of whole sample-frames")
        clen[j] = c.numel() // step
    have = clen[:n_clips].astype(np.int64) + np.diff(so)
    if n_rows:
        if ((rc < 0) | (rc >= n_clips)).any():
            raise ValueError("row_clip names a clip that is not there")
        if ((ra < 0) | (ra > have[rc] - row_len)).any():         # (not ra + row_len > have: that sum can wrap)
            raise ValueError("a row does not end inside its clip")
    na = np.zeros(max(n_clips, 1), np.int64)
    if nxt is not None:
        if next_at is None or len(nxt) != n_clips or len(next_at) != n_clips:
            raise ValueError("nxt and next_at need one entry per clip")
        na[:n_clips] = np.ascontiguousarray(next_at, np.int64).reshape(-1)
        if ((na[:n_clips] < 0) | (na[:n_clips] > have)).any():
            raise ValueError("0 <= next_at[j] <= the clip's sample-frames")
        for j, t in enumerate(nxt):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or t.numel() != (have[j] - na[j]) * step:
                raise ValueError(f"nxt[{j}] must be a 1-D uint8 tensor of {(have[j] - na[j]) * step} bytes")
    # ---- the device's side: everything on one device, no remainder over anything that is read
    _require_device_tensor(src, "src")
    device = src.device
    spans = [(src.data_ptr(), src.numel())] if src.numel() else []
    for j, c in enumerate(carry):
        if c is not None and c.numel():
            _require_device_tensor(c, f"carry[{j}]")
            if c.device != device:
                raise ValueError("the carries must live on the device of src")
            ptrs[0, j] = c.data_ptr()
            spans.append((c.data_ptr(), c.numel()))
    if nxt is not None:
        spans.sort()
        starts = np.array([s for s, _ in spans], np.uint64)
        ends = np.array([s + n for s, n in spans], np.uint64)
        for j, t in enumerate(nxt):
            if t is None or not t.numel():
                continue
            _require_device_tensor(t, f"nxt[{j}]")
            if t.device != device:
                raise ValueError("the remainders must live on the device of src")
            ptrs[1, j] = a = t.data_ptr()
            if starts.size and ((starts < np.uint64(a + t.numel())) & (ends > np.uint64(a))).any():
                raise ValueError(f"nxt[{j}] overlaps src or a carry")
    out = torch.empty((n_rows, row_len * step), dtype=torch.uint8, device=device)
    if n_clips == 0 or (n_rows == 0 and not ptrs[1].any()):
        return out
    # the seven tables in one upload: int64 carry_ptr | src_off | row_at | next_at | next_ptr, int32 carry_len | row_clip
    parts = [ptrs[0, :n_clips], so, ra, na[:n_clips], ptrs[1, :n_clips], clen[:n_clips], rc]
    dev = torch.from_numpy(np.concatenate([np.ascontiguousarray(a).view(np.uint8) for a in parts])).to(device)
    at = np.cumsum([0] + [a.nbytes for a in parts])
    p = [dev.data_ptr() + int(o) for o in at[:-1]]
    base = src.data_ptr() if src.numel() else dev.data_ptr()    # (every span empty: nothing is read through it)
    with torch.cuda.device(device):
        _lib.load().clips_carry_cut(p[0], p[5], base, p[1], n_clips, p[6], p[2], n_rows, row_len, step, out.data_ptr() if n_rows else 0,
                                    p[3], p[4] if nxt is not None else 0, _stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------
# raw DEFLATE inflate (frad_inflate_raw): the zlib.decompress(frad, wbits=-15) of profile1.py:59 / profile2.py:61-64
# ---------------------------------------------------------------------------------------------
INFLATE_OK, INFLATE_INVALID, INFLATE_OVERFLOW = 0, 1, 2


def inflate_batch(src: torch.Tensor, offsets: torch.Tensor, dst_stride: int):
    """Raw DEFLATE decode of a batch of independent streams on the device (RFC 1951, no wrapper, no dictionary).

    ``src`` uint8 [total], ``offsets`` int64 [n_frames + 1] (both CUDA tensors): stream i is ``src[offsets[i]:offsets[i+1]]``.
    Returns ``(dst uint8 [n_frames, dst_stride], dst_bytes int64 [n_frames], status int32 [n_frames])``: with status 0 row i's
    first ``dst_bytes[i]`` bytes equal ``zlib.decompress(stream_i, wbits=-15)``; status 1 = zlib rejects the stream, 2 = the
    output would exceed ``dst_stride`` bytes.  ``dst_stride`` a positive multiple of 16.  The offsets are checked against
    ``src`` here (one device-to-host read), so no caller buffer reaches the kernel unchecked."""
    n_frames = _require_ragged(src, offsets, "src")
    dst_stride = int(dst_stride)
    if dst_stride < 16 or dst_stride % 16:
        raise ValueError(f"dst_stride must be a positive multiple of 16, got {dst_stride}")
    _require_frame_count(n_frames, "streams")
    _require_offsets_within(src, offsets)
    # + 16 bytes behind the last row: frad_rows_compact reads a row as aligned words, one word beyond its bytes
    dst = torch.empty(n_frames * dst_stride + 16, dtype=torch.uint8, device=src.device)
    nbytes = torch.empty(max(n_frames, 1), dtype=torch.int64, device=src.device)
    status = torch.empty(max(n_frames, 1), dtype=torch.int32, device=src.device)
    if n_frames:
        base = src.data_ptr() if src.numel() else dst.data_ptr()   # (every stream empty: nothing is read)
        with torch.cuda.device(src.device):
            _lib.load().inflate_raw(base, offsets.data_ptr(), n_frames, dst.data_ptr(), dst_stride, nbytes.data_ptr(),
                                    status.data_ptr(), _stream_ptr())
    return dst[:n_frames * dst_stride].view(n_frames, dst_stride), nbytes[:n_frames], status[:n_frames]


# ---------------------------------------------------------------------------------------------
# raw DEFLATE deflate (frad_deflate_raw): the zlib.compress(frad, wbits=-15) of profile1.py:50 / profile2.py:54
# ---------------------------------------------------------------------------------------------
DEFLATE_OK, DEFLATE_HOST, DEFLATE_OVERFLOW = 0, 1, 2
DEFLATE_LIMIT = 65274            # wsize + MAX_DIST: bodies from this length on get DEFLATE_HOST


def deflate_batch(src: torch.Tensor, offsets: torch.Tensor):
    """zlib's raw deflate (level 6, memLevel 8, 15 window bits, default strategy) of a batch of bodies on the device.

    ``src`` uint8 [total], ``offsets`` int64 [n_frames + 1] (both CUDA tensors): body i is ``src[offsets[i]:offsets[i+1]]``.
    Returns ``(dst uint8 [n_frames, stride], dst_bytes int64 [n_frames], status int32 [n_frames])``: with status 0 row i's
    first ``dst_bytes[i]`` bytes equal ``zlib.compressobj(-1, zlib.DEFLATED, -15)``'s ``compress(body) + flush()``; status 1
    (``DEFLATE_HOST``) = the body is ``DEFLATE_LIMIT`` bytes or longer and is left to the host (nothing written to its row).
    The stride is chosen from the longest body, with 4 bytes to spare for ``frad_rows_compact``'s word reads.  The offsets
    are checked against ``src`` here (one device-to-host read), so no caller buffer reaches the kernel unchecked."""
    n_frames = _require_ragged(src, offsets, "src")
    _require_frame_count(n_frames, "bodies")
    longest = (offsets[1:] - offsets[:-1]).max() if n_frames else torch.zeros((), dtype=torch.int64, device=src.device)
    longest, = _require_offsets_within(src, offsets, longest)             # (the longest body rides along in the one host read)
    lib = _lib.load()
    stride = lib.deflate_stride(min(longest, DEFLATE_LIMIT - 1) + 4)
    dst = torch.empty(max(n_frames * stride, 16), dtype=torch.uint8, device=src.device)
    nbytes = torch.empty(max(n_frames, 1), dtype=torch.int64, device=src.device)
    status = torch.empty(max(n_frames, 1), dtype=torch.int32, device=src.device)
    if n_frames:
        base = src.data_ptr() if src.numel() else dst.data_ptr()   # (every body empty: nothing is read)
        with torch.cuda.device(src.device):
            lib.deflate_raw(base, offsets.data_ptr(), n_frames, dst.data_ptr(), stride, nbytes.data_ptr(), status.data_ptr(),
                            _stream_ptr())
    return dst[:n_frames * stride].view(n_frames, stride), nbytes[:n_frames], status[:n_frames]
