// One read of a counted row, added with the lanes of the wave that agree (uint_traces.hip, ec_traces.hip).
//
// Most relations of a session share their bound, and many an operand (the x of a Horner evaluation); all points and live additions of a
// session hit one group's counter.  A lane per relation would send a wave's 64 atomics to ONE address, and they serialise (measured:
// 0.56 ms for 49 159 rows that read one bound).  So the lanes of the wave that are here compare their counter with the first lane's;
// those that agree add once, the rest add for themselves.
#pragma once
#include "gl.cuh"

__host__ __device__ __forceinline__ void wave_count(u32* counter) {
#ifdef __HIP_DEVICE_COMPILE__
  const unsigned long long here = __ballot(1);
  const int first = __ffsll(here) - 1;
  const unsigned long long mine = (unsigned long long)counter;
  const unsigned long long lead = ((unsigned long long)(u32)__shfl((int)(mine >> 32), first) << 32) | (u32)__shfl((int)(u32)mine, first);
  const unsigned long long same = __ballot(mine == lead);
  if (mine != lead) atomicAdd(counter, 1u);
  else if ((int)__lane_id() == first) atomicAdd(counter, (u32)__popcll(same));
#else
  ++*counter;
#endif
}
