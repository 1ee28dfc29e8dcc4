// ed_build_kernels.hpp — the non-template kernels of the H builders
// (ed_build.hip, the only unit that includes this header, so each is compiled
// once): the basis map, the SELL-64 row counts and their scan, the value
// dictionaries of the packed form, and segment A of the two-segment form.
//   k_build_map    H%map from the (off, rank) tables        build_sector ED_SETUP.f90:886-984
//   k_count        elements per row + SELL-64 slice width   ed_buildH_c pass 1
#pragma once
#include "ed_kernels.hpp"
#include "ed_split.hpp"

namespace edg {

// ------------------------------------------------------------- basis / map
static __global__ void __launch_bounds__(kBlock) k_build_map(const int64_t* __restrict__ blk_off,
                                                      const uint32_t* __restrict__ blk_idw, int nblk,
                                                      const int32_t* __restrict__ need_cls,
                                                      const uint32_t* __restrict__ by_cls,
                                                      const int32_t* __restrict__ cls_start, int ns,
                                                      int64_t dim, uint32_t* __restrict__ map) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < dim;
       i += (int64_t)gridDim.x * kBlock) {
    int lo = 0, hi = nblk;  // blk_off[lo] <= i < blk_off[hi]
    while (hi - lo > 1) {
      int mid = (lo + hi) >> 1;
      if (blk_off[mid] <= i) lo = mid;
      else hi = mid;
    }
    uint32_t idw = blk_idw[lo];
    uint32_t iup = by_cls[cls_start[need_cls[idw]] + (i - blk_off[lo])];
    map[i] = iup | (idw << ns);
  }
}

// ------------------------------------------------------------ stored build
struct CountAcc {
  int n = 0;
  __device__ __forceinline__ void diag(double, double) {}
  __device__ __forceinline__ void off(uint32_t, double, double) { n++; }
};

// cnt[i] = off-diagonal elements of row i; width[s] = max over slice s.
static __global__ void __launch_bounds__(kBlock) k_count(const EdModel* __restrict__ Mp,
                                                  const uint32_t* __restrict__ map, int64_t dim,
                                                  int64_t nslice, uint16_t* __restrict__ cnt,
                                                  int32_t* __restrict__ width) {
  const EdModel& M = *Mp;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nslice * 64;
       i += (int64_t)gridDim.x * kBlock) {
    int c = 0;
    if (i < dim) {
      CountAcc a;
      gen_row(M, map[i], a);
      c = a.n;
      cnt[i] = (uint16_t)c;
    }
    int w = wave_max(c);
    if ((threadIdx.x & 63) == 0) width[i >> 6] = w;
  }
}

// Exclusive scan of 64*width -> sptr (int64), three-pass.
// *out += sum of n 16-bit counts (grid-strided; wave sums, one atomic per wave)
static __global__ void __launch_bounds__(kBlock) k_sum_u16(const uint16_t* __restrict__ c, int64_t n,
                                                    unsigned long long* out) {
  unsigned long long acc = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) acc += c[i];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}

static __global__ void __launch_bounds__(1024) k_scan_blocks(const int32_t* __restrict__ width, int64_t n,
                                                      int64_t* __restrict__ out,
                                                      int64_t* __restrict__ bsum) {
  __shared__ int64_t s[1024];
  int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
  int64_t x = (i < n) ? 64 * (int64_t)width[i] : 0;
  s[threadIdx.x] = x;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    int64_t t = (threadIdx.x >= (unsigned)o) ? s[threadIdx.x - o] : 0;
    __syncthreads();
    s[threadIdx.x] += t;
    __syncthreads();
  }
  if (i < n) out[i] = s[threadIdx.x] - x;  // exclusive within block
  if (threadIdx.x == 1023) bsum[blockIdx.x] = s[1023];
}
static __global__ void k_scan_spine(int64_t* __restrict__ bsum, int64_t nb, int64_t* __restrict__ total) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int64_t acc = 0;
    for (int64_t b = 0; b < nb; b++) {
      int64_t t = bsum[b];
      bsum[b] = acc;
      acc += t;
    }
    *total = acc;
  }
}
static __global__ void __launch_bounds__(1024) k_scan_add(int64_t* __restrict__ out, int64_t n,
                                                   const int64_t* __restrict__ bsum,
                                                   const int64_t* __restrict__ total) {
  int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
  if (i < n) out[i] += bsum[blockIdx.x];
  if (i == 0) out[n] = *total;
}

// ------------------------------------------- packed form: the dictionary
// Insert every value's bit pattern; plain reads first so that the few
// distinct keys cost one CAS each, not one per slot.
// Wave-level deduplication before the table: the lanes of a wavefront read 64
// consecutive SELL slots, which hold only a few distinct values (hoppings);
// one leader per distinct key goes to the table.  Without it every slot did a
// read (and the first ones a CAS) of the same few table lines: all of the
// device's requests on one L2 channel (N28: 1.05 ms; c4 farm: 0.75 ms per
// sector, 0.125 s of the serial configs[3] farm).
__device__ __forceinline__ bool wave_key_leader(unsigned long long key) {
  const int lane = threadIdx.x & 63;
  unsigned long long pending = __ballot(1);
  bool lead = false;
  while (pending) {
    const int l = __ffsll((long long)pending) - 1;
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)key, l);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(key >> 32), l);
    const unsigned long long kl = ((unsigned long long)hi << 32) | lo;
    const unsigned long long same = __ballot(key == kl);
    lead |= lane == l;
    pending &= ~same;
  }
  return lead;
}

static __global__ void __launch_bounds__(kBlock) k_dict_insert(const double* __restrict__ vals, int64_t n,
                                                        unsigned long long* table,
                                                        unsigned int* overflow) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const unsigned long long key = (unsigned long long)__double_as_longlong(vals[i]);
    if (!wave_key_leader(key)) continue;
    if (key == kDictEmpty) {
      atomicOr(overflow, 1u);
      continue;
    }
    uint32_t h = dict_hash(key);
    bool done = false;
    for (int probe = 0; probe < kDictTable && !done; probe++) {
      const unsigned long long cur = ((volatile unsigned long long*)table)[h];
      if (cur == key) {
        done = true;
      } else if (cur == kDictEmpty) {
        const unsigned long long prev = atomicCAS(table + h, kDictEmpty, key);
        if (prev == kDictEmpty || prev == key) done = true;
        else h = (h + 1) & (kDictTable - 1);  // lost the race to another key: probe on
      } else {
        h = (h + 1) & (kDictTable - 1);
      }
    }
    if (!done) atomicOr(overflow, 1u);
  }
}

static __global__ void __launch_bounds__(kBlock) k_dict_pack(const int32_t* __restrict__ cols,
                                                      const double* __restrict__ vals, int64_t n,
                                                      const unsigned long long* __restrict__ table,
                                                      const uint8_t* __restrict__ tidx,
                                                      uint32_t* __restrict__ words) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const unsigned long long key = (unsigned long long)__double_as_longlong(vals[i]);
    uint32_t h = dict_hash(key);
    while (table[h] != key) h = (h + 1) & (kDictTable - 1);  // present by construction
    words[i] = (uint32_t)cols[i] | ((uint32_t)tidx[h] << kPackShift);
  }
}

// Complex H (the reference's complex(8) arithmetic, ED_SPARSE_MATRIX.f90:11-29):
// the same words over a dictionary of distinct (re, im) pairs.  Keys are a
// 64-bit mix of the two bit patterns; the inserting thread records the pair,
// and the pack kernel checks every slot's pair bit for bit against its entry
// (a hash collision between two pairs flags overflow: the plain arrays serve).
__device__ __forceinline__ unsigned long long pair_key(double2 v) {
  unsigned long long a = (unsigned long long)__double_as_longlong(v.x);
  unsigned long long b = (unsigned long long)__double_as_longlong(v.y);
  unsigned long long k = a ^ (b * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull + (a << 6) + (a >> 2));
  return k == kDictEmpty ? 0x7ff8dead00000001ull : k;
}

static __global__ void __launch_bounds__(kBlock) k_dict_insert_c(const double2* __restrict__ vals, int64_t n,
                                                          unsigned long long* table, double2* reps,
                                                          unsigned int* overflow) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const double2 v = vals[i];
    const unsigned long long key = pair_key(v);
    if (!wave_key_leader(key)) continue;  // (pairs with equal keys are checked at pack time)
    uint32_t h = dict_hash(key);
    bool done = false;
    for (int probe = 0; probe < kDictTable && !done; probe++) {
      const unsigned long long cur = ((volatile unsigned long long*)table)[h];
      if (cur == key) {
        done = true;
      } else if (cur == kDictEmpty) {
        const unsigned long long prev = atomicCAS(table + h, kDictEmpty, key);
        if (prev == kDictEmpty) {
          reps[h] = v;  // the inserting thread records the pair
          done = true;
        } else if (prev == key) {
          done = true;
        } else {
          h = (h + 1) & (kDictTable - 1);
        }
      } else {
        h = (h + 1) & (kDictTable - 1);
      }
    }
    if (!done) atomicOr(overflow, 1u);
  }
}

static __global__ void __launch_bounds__(kBlock) k_dict_pack_c(const int32_t* __restrict__ cols,
                                                        const double2* __restrict__ vals, int64_t n,
                                                        const unsigned long long* __restrict__ table,
                                                        const double2* __restrict__ reps,
                                                        const uint8_t* __restrict__ tidx,
                                                        uint32_t* __restrict__ words,
                                                        unsigned int* overflow) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const double2 v = vals[i];
    const unsigned long long key = pair_key(v);
    uint32_t h = dict_hash(key);
    while (table[h] != key) h = (h + 1) & (kDictTable - 1);  // present by construction
    const double2 r = reps[h];
    if (__double_as_longlong(r.x) != __double_as_longlong(v.x) ||
        __double_as_longlong(r.y) != __double_as_longlong(v.y))
      atomicOr(overflow, 1u);
    words[i] = (uint32_t)cols[i] | ((uint32_t)tidx[h] << kPackShift);
  }
}

// ------------------------------------- two-segment form (ed_split.hpp)
// ---- build: segment A
// nA[i] = in-block elements of row i; widthA[s] = max over slice s.  Also the
// largest cross-block count of any row (atomicMax into *farmax).
static __global__ void __launch_bounds__(kBlock) k_split_count_a(const int64_t* __restrict__ sptr,
                                                          const uint32_t* __restrict__ words,
                                                          const uint16_t* __restrict__ cnt,
                                                          const uint32_t* __restrict__ map, int ns,
                                                          int64_t dim, int64_t nslice, uint16_t* __restrict__ na,
                                                          int32_t* __restrict__ widthA, int* farmax) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nslice * 64;
       i += (int64_t)gridDim.x * kBlock) {
    int c = 0, f = 0;
    if (i < dim) {
      const uint32_t blk = map[i] >> ns;
      const uint32_t* wp = words + sptr[i >> 6] + (i & 63);
      const int n = cnt[i];
      for (int k = 0; k < n; k++) {
        const uint32_t col = wp[64 * k] & kPackColMask;
        if ((map[col] >> ns) == blk) c++;
        else f++;
      }
      na[i] = (uint16_t)c;
    }
    const int w = wave_max(c);
    const int fm = wave_max(f);
    if ((threadIdx.x & 63) == 0) {
      widthA[i >> 6] = w;
      atomicMax(farmax, fm);
    }
  }
}

static __global__ void __launch_bounds__(kBlock) k_split_fill_a(const int64_t* __restrict__ sptr,
                                                         const uint32_t* __restrict__ words,
                                                         const uint16_t* __restrict__ cnt,
                                                         const uint32_t* __restrict__ map, int ns,
                                                         int64_t dim, int64_t nslice,
                                                         const int64_t* __restrict__ sptrA,
                                                         uint32_t* __restrict__ wordsA, uint32_t zpad) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nslice * 64;
       i += (int64_t)gridDim.x * kBlock) {
    const int64_t s = i >> 6;
    const int wA = (int)((sptrA[s + 1] - sptrA[s]) >> 6);
    uint32_t* ap = wordsA + sptrA[s] + (i & 63);
    int k2 = 0;
    if (i < dim) {
      const uint32_t blk = map[i] >> ns;
      const uint32_t* wp = words + sptr[s] + (i & 63);
      const int n = cnt[i];
      for (int k = 0; k < n; k++) {
        const uint32_t wd = wp[64 * k];
        if ((map[wd & kPackColMask] >> ns) == blk) ap[64 * (k2++)] = wd;
      }
    }
    // padding: own column (or 0 past the last row), the dictionary's zero
    const uint32_t pad = (uint32_t)(i < dim ? i : 0) | zpad;
    for (; k2 < wA; k2++) ap[64 * k2] = pad;
  }
}

}  // namespace edg
