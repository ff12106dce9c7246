// The order-preserving unsigned 64-bit keys of virtual dictionaries (pg_vdict.hip), shared with the kernels that produce such keys from
// something other than a stored column (pg_kernels_exprkey.hip).  Equality follows the reference's fastutil maps: FLOAT / DOUBLE compare by
// floatToIntBits / doubleToLongBits (every NaN is one key, -0.0 and 0.0 are two); unsigned order of the keys is value order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// kind: 0 INT, 1 LONG, 2 FLOAT, 3 DOUBLE; `bits`: the value's bits, native endian, in the low bytes
__device__ __host__ inline uint64_t pg_vdict_key_of_bits(uint64_t bits, int kind) {
  switch (kind) {
    case 0: return (uint64_t)(int64_t)(int32_t)(uint32_t)bits ^ (1ULL << 63);
    case 1: return bits ^ (1ULL << 63);
    case 2: {
      uint32_t f = (uint32_t)bits;
      if ((f & 0x7FFFFFFFu) > 0x7F800000u) f = 0x7FC00000u;          // floatToIntBits: one NaN
      return (uint64_t)(f ^ ((f >> 31) ? 0xFFFFFFFFu : 0x80000000u));
    }
    default: {
      uint64_t d = bits;
      if ((d & 0x7FFFFFFFFFFFFFFFULL) > 0x7FF0000000000000ULL) d = 0x7FF8000000000000ULL;
      return d ^ ((d >> 63) ? ~0ULL : (1ULL << 63));
    }
  }
}
