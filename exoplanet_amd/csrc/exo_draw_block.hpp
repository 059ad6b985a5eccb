// exo_draw_block.hpp -- what the one-workgroup-per-draw likelihood kernels share: the width of a draw's workgroup (the
// radial-velocity and the astrometric likelihood: exo_rv_like_core.hpp, exo_astrometry_core.hpp re-export the names) and the
// sum over a wave in a fixed order (those two, exo_noise.hip and exo_estimators.hip).  The constants compile for gfx950 and
// for the host (EXO_HOST_BUILD: the harnesses under tests/); the shuffle is device code only.
#pragma once
#include <stdint.h>

#ifndef EXO_HOST_BUILD
#include <hip/hip_runtime.h>
#endif

namespace exo {
namespace draw {

constexpr int kWave = 64;
constexpr int kNarrowCad = 128;   // up to this many epochs one wave takes the draw, above four do
constexpr int kNarrow = 64, kWide = 256;

// the width of a draw's workgroup: from the length of the series alone, never from the number of draws
constexpr int block_threads(int64_t n_cad) { return n_cad <= kNarrowCad ? kNarrow : kWide; }

#ifndef EXO_HOST_BUILD
// the sum of a wave's 64 lanes, valid in lane 0: a shuffle-down tree, the same order every time
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
  return v;
}
#endif

}  // namespace draw
}  // namespace exo
