// The wave-specialised 256 x 128 x 64 prefill tile that gemm3.hip and bitgemm.hip share: the definitions both units (host and device side)
// name.  The kernel text they share -- the staging waves' schedule, the matrix waves, the split-K hand-off and the epilogue -- is
// tile256_body.inc, included into the body of both kernels.
#pragma once
#include "common.hpp"

namespace qllm {
namespace tile256 {

constexpr int BM = 256, BN = 128, BK = 64;
constexpr int kATile = BM * BK, kBTile = BN * BK;  // halves per stage
constexpr size_t kLdsBytes = (size_t)(3 * kATile + 2 * kBTile) * sizeof(half_t);  // A ring 3 x 32 KB + B 2 x 16 KB = 128 KB, dynamic only
typedef float float16_t __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void_t;

// LDS rows are 64 halves (128 B) whose eight 16-byte slots are XORed by lds_row_swizzle(row)
__device__ __forceinline__ int tile_off(int row, int slot) { return row * BK + ((slot ^ lds_row_swizzle(row)) & 7) * 8; }  // in halves

// each XCD (block id % 8) walks a contiguous run of the n blocks
__device__ __forceinline__ int xcd_run(int b, int n) {
  const int q = n / 8, r = n % 8, xcd = b % 8, idx = b / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

}  // namespace tile256
}  // namespace qllm
