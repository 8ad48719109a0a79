// frad_platform.hpp -- the one seam between the kernels and the toolchain.
//
// Product build (hipcc --offload-arch=gfx950): the real HIP runtime.  The kernels are written for
// gfx950 only: wave64, LDS, no portability layer.
// Test build (g++ -DFRAD_HOST_EMULATION, tests/emu/): the same kernel source runs under a small
// thread-per-lane interpreter so that indexing and packing logic can be checked -- and run under
// AddressSanitizer, which the GPU pool does not offer -- in the CPU-only build container.  The
// emulator is test infrastructure and is never linked into libfrad_hip.so.
//
// Everything that one of the two toolchains does not understand -- gfx950 builtins, inline assembly,
// address spaces, scoped atomics, nontemporal accesses -- is a primitive of this seam, with two
// definitions: frad_platform_gfx950.hpp (the product's) and frad_platform_emu.hpp (the emulator's, on top
// of the interpreter in tests/emu/hip_emu.hpp).
// The #ifdef below is the only test of FRAD_HOST_EMULATION in the kernel sources (one documented
// exception: the LDS staging of k_p4_pack, frad_kernels.hpp), and apart from the
// three calls that hip_emu.hpp provides under their own names (__builtin_amdgcn_sched_barrier, _fence,
// _wave_barrier) no builtin and no asm statement appears outside the gfx950 file.  The contracts are
// written once, here.  "Exact" primitives return the same bits from both definitions on the stated
// domain; tests/test_lane_prims.py runs one kernel of them (frad_debug_lane_prims, frad_util.hip) on
// both builds against a NumPy model.  A lane is threadIdx.x & 63, a wave the 64 lanes of equal
// threadIdx.x >> 6; "uniform" = the same value in every lane of the wave.
//
// ---- exact: lane movement and reductions (every lane of the wave must make the call) -------------------
//   FRAD_ROWS16_ALLREDUCE_U64(v, op)
//                                 v (a u64 variable) = butterfly all-reduce inside each row of 16 lanes: four steps, in
//                                 which a lane combines op(own, partner's) with the partner at lane xor 1, 2, 4, 8.  (gfx950:
//                                 DPP quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror; the mirrors'
//                                 partners hold the same value as the xor partners once the smaller groups are
//                                 uniform.)  Domain: op commutative in its bits (op(a, b) == op(b, a)), which makes
//                                 every group uniform after its step; any 64-bit patterns.
//   wave_row_u64(v, row)          v of lane 16 * row, uniform; row a compile-time-known 0 .. 3
//   wave_read_lane(v, src)        v (int) of lane src; src uniform, 0 .. 63
//   wave_uniform_int(v)           v (int) of the first lane; the kernels pass values that are uniform already (it
//                                 tells the compiler so: the value and what is derived from it stay in SGPRs), and
//                                 that is the domain: all 64 lanes active
//   wave_any(b)                   true in every lane iff b is true in some lane (gfx950: one ballot)
//   The reductions in frad_common.hpp (wave_allreduce_u64, half_wave_max_u64, half_wave_sum_f64) are plain code
//   over the first two: rows, then op(op(row 0, row 1), op(row 2, row 3)) or the two halves' op(row, row).
// ---- exact: bits ----------------------------------------------------------------------------------------
//   bfe_u32(word, shift, width)   bits [shift, shift + width) of word, zero-extended    } 0 <= shift < 32, 0 < width < 32;
//   bfe_i32(word, shift, width)   the same field, sign-extended from its top bit        } a field that would pass bit 31
//                                 ends there (the kernels stay below: shift + width <= 32)
//   wave_perm(v, sel)             byte i of the result = byte (selector byte i) - 4 of v.  Domain: selector bytes
//                                 4 .. 7 (v_perm_b32 addresses its second source with 0 .. 3 and constants with
//                                 >= 8: no kernel uses either, the emulator returns 0 for them)
// ---- exact: arithmetic ------------------------------------------------------------------------------------
//   absmax_acc(fm, v)             fm = max(fm, |v|) as one v_max_f64.  Domain: fm >= +0 and not NaN (a running
//                                 maximum that starts at 0); any v, a NaN v leaves fm as it is
//   fma_free(s, b, a)             fma(s, b, a), one rounding, in a register of its own.  Domain: every float64
//                                 (denormals are kept); of a NaN result only "is a NaN" is common to both
//   nonfinite_f32(f)              f is +-Inf or a NaN (v_cmp_class_f32, mask 0x207)
// ---- exact: memory and waits ------------------------------------------------------------------------------
//   lds_dma16<AUX>(src, lds)      16 bytes per lane from global memory straight into LDS, no register:
//                                 lane t's src[0 .. 16) lands at lds + 16 t (global_load_lds_dwordx4).  src per
//                                 lane and 16-byte aligned, lds uniform and 16-byte aligned, AUX the cache policy
//                                 bits.  Asynchronous: complete after FRAD_VMCNT and a team_sync<64>()
//   FRAD_VMCNT(n)                 wait until at most n (a constant expression) of this wave's vector-memory
//                                 operations are in flight; nothing on the emulator, whose accesses complete in
//                                 program order
//   FRAD_LGKM0()                  this wave's LDS (and scalar) accesses have completed; a full fence on the emulator
//   FRAD_LDS_BARRIER()            workgroup barrier that only waits for this wave's LDS traffic: __syncthreads() also
//                                 drains vmcnt, i.e. every global load and store in flight, which is exactly what a
//                                 pipelined kernel must not do
//   FRAD_LDS_ADD(p, v)            atomic fetch-add on an LDS word, workgroup scope, returns the old value
//   FRAD_LDS_LOAD(p)              atomic load of an LDS word, workgroup scope
//   FRAD_NAP(n)                   give way for about 64 n cycles (s_sleep; the emulator yields its thread)
//   FRAD_NT_LOAD(p)               } streaming (nontemporal) access to data touched once: the value is that of a plain
//   FRAD_NT_STORE(v, p)           } access, which is what the emulator makes
//   FRAD_DYN_SMEM(name)           the block's dynamic LDS, 16-byte aligned, as unsigned char name[]
//   FRAD_GPTR(T, p), FRAD_GCPTR   a pointer that went through a real (noinline) call is "generic" to the compiler and
//                                 gets FLAT instructions, which also count on lgkmcnt -- an LDS-only wait would then
//                                 wait for global stores.  These casts put device-memory pointers back into the
//                                 global address space.
// ---- no value: what the optimiser and the tools see ---------------------------------------------------------
//   FRAD_OPAQUE(x)                make a lane value opaque to the optimiser (used to stop loop-invariant code motion
//                                 from parking hundreds of per-lane LDS addresses in VGPRs across a persistent loop)
//   FRAD_PIN(x)                   the value is complete at this point of the instruction stream: pure arithmetic
//                                 otherwise floats across scheduling fences
//   FRAD_CLOCK()                  the shader clock (s_memtime), diagnostic builds only; 0 on the emulator
//   FRAD_ASM_COMMENT(text)        a comment in the assembly, no instruction -- but a statement the scheduler will not
//                                 move code across; nothing on the emulator
//   __launch_bounds__(...)        HIP's own attribute; expands to nothing on the emulator
// ---- approximate float32 instructions -----------------------------------------------------------------------
//   p1w_sqrtf(v)  k7_log2f(v)  k7_exp2f(v)  k7_rcpf(v)
//                                 v_sqrt_f32, v_log_f32, v_exp_f32, v_rcp_f32: about 1 ulp, NOT bit-equal to libm's
//                                 sqrtf / log2f / exp2f / division, which the emulator calls.  The kernels use them
//                                 for seeds and decisions only, never for a stored value, and re-decide exactly
//                                 whatever lies within the error bound of a boundary; tests/test_p1_exact.py checks
//                                 that end to end on both builds.  They are not part of the parity test.
#pragma once
#include <stdint.h>

namespace frad {
typedef unsigned long long u64;
// plain compiler vectors for 8/16-byte global accesses (HIP's uint4/double2 are classes and cannot be
// accessed through an address-space qualified pointer)
typedef uint32_t v4u __attribute__((vector_size(16)));
typedef uint32_t v2u __attribute__((vector_size(8)));
typedef double v2d __attribute__((vector_size(16)));
}  // namespace frad

#ifdef FRAD_HOST_EMULATION
#include "hip_emu.hpp"
#include "frad_platform_emu.hpp"
#else
#include "frad_platform_gfx950.hpp"
#endif
