// Philox-4x32-10 (Salmon et al., SC'11): counter-based, so any element's draw is recomputable.
// The generator of head_ops.hip (philox_u32 there) and of reference.philox_u32, with all four words
// of one counter returned: counter (ctr lo, ctr hi, offset, 0), key = seed.
#pragma once

namespace dbx {

__device__ __forceinline__ void philox4x32_10(unsigned long long ctr, unsigned long long seed, unsigned offset,
                                              unsigned (&w)[4]) {
  unsigned c0 = (unsigned)ctr, c1 = (unsigned)(ctr >> 32), c2 = offset, c3 = 0u;
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

}  // namespace dbx
