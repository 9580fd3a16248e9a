// The split-f16 tile-image path (x3_impl.h), instantiated for the two model widths of the reference's configurations:
//   namespace x3: d = 256, 8 heads of 32 (the north star's d_model >= 256 variant of location_finding): 8 waves per workgroup, one
//                 16-row token tile per wave, two waves per SIMD (256 registers each);
//   namespace x5: d = 512, 8 heads of 64 (config/task/psychometric.yaml with d_model = 512): a token tile's input fragments (128
//                 registers) and accumulators (128) do not fit a 256-register wave, so a workgroup is 4 waves -- one per SIMD --
//                 with the whole 512-entry register file of their SIMD lane (accumulators in the AGPR half).
//   namespace x1: d = 128, 4 heads of 32 (the first width above the reference's d = 32): the images, the key list, the weight stream
//                 and the attention of x3_impl.h at this width; a k-step is half a 16-pair chunk, so the weight layout and the
//                 kernels that walk it are x1.h's (X3_PAIRED): 8 waves per workgroup, TWO token tiles per wave.
#pragma once
#include "tile_image.h"

// Kernels added since round 4 are compiled without the packed fp32 instructions (v_pk_add / mul / fma_f32): a per-kernel target
// attribute, so that the kernels from before keep the code they have.  (Device pass only: the host compiler does not know the feature.)
#if defined(__HIP_DEVICE_COMPILE__)
#define X3_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define X3_NO_PK_F32
#endif

#define X3_NS x3
#define X3_D 256
#define X3_HD 32
#define X3_THREADS 512
#define X3_KV_AHEAD 1
#define X3_LONGKEYS 1      // rollouts with 65 .. 160 visible keys: the long-key variants (x3_impl.h, KV_EP)
#ifndef X3_ILV256
#define X3_ILV256 1
#endif
#define X3_INTERLEAVE X3_ILV256
#define X3_PAIRED 0
#include "x3_impl.h"
#undef X3_NS
#undef X3_D
#undef X3_HD
#undef X3_THREADS
#undef X3_KV_AHEAD
#undef X3_LONGKEYS
#undef X3_INTERLEAVE
#undef X3_PAIRED

#define X3_NS x5
#define X3_D 512
#define X3_HD 64
#define X3_THREADS 256
#define X3_LONGKEYS 0      // (one wave per SIMD with its register file full: 64 keys at most)
#ifndef X5_KV_AHEAD
#define X5_KV_AHEAD 1
#endif
#define X3_KV_AHEAD X5_KV_AHEAD
#ifndef X3_ILV512
#define X3_ILV512 1
#endif
#define X3_INTERLEAVE X3_ILV512
#define X3_PAIRED 0
#include "x3_impl.h"
#undef X3_NS
#undef X3_D
#undef X3_HD
#undef X3_THREADS
#undef X3_KV_AHEAD
#undef X3_LONGKEYS
#undef X3_INTERLEAVE
#undef X3_PAIRED

#define X3_NS x1
#define X3_D 128
#define X3_HD 32
#define X3_THREADS 512
#define X3_KV_AHEAD 1
#define X3_LONGKEYS 0      // (64 keys at most)
#define X3_INTERLEAVE 1
#define X3_PAIRED 1
#include "x3_impl.h"
#undef X3_NS
#undef X3_D
#undef X3_HD
#undef X3_THREADS
#undef X3_KV_AHEAD
#undef X3_LONGKEYS
#undef X3_INTERLEAVE
#undef X3_PAIRED
