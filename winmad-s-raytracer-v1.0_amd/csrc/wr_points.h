// Point sets on the device (include/winmad_rt.h wr_points_*): a
// hashed grid over a caller's points that answers KdTree::searchInRadius and
// KdTree::searchKnn (scene/KDtree.h:141-208) exactly.  Included by
// wr_render.hip inside its anonymous namespace, after wr_shade.h.  The ideas
// are those of the VCM merge grid (wr_vcm.h); nothing is shared with it.
//
// Definition (never a function of the grid): d2(q, p) = sqr_len(q - p) in
// float, each step rounded (-ffp-contract=off).  A radius query reports p iff
// sqrtf(d2) < r (sqrtf correctly rounded, as on the host); a k-nearest query
// takes the points with d2 < max_sqr_dist and keeps the k smallest (d2, index).
//
// Index: the points with three finite coordinates, as records {pos, index} of
// 16 bytes, sorted by bucket -- a stable radix sort of (bucket, index), so the
// record order, and with it every output, is a pure function of the input
// array.  start[b] .. start[b + 1] are the records of bucket b.  A grid row
// (cy, cz) is hashed to a run of kPtsRowW buckets, one per cx mod kPtsRowW, so
// the cells [x0, x1] of a row are one contiguous bucket range (two where cx
// wraps).  A bucket may hold several cells: a scan takes a record only in the
// record's own cell, so no point is reported twice.
//
// Cover: the cell of a coordinate is floor((x - org) / cell), clamped; float
// subtraction, division and floor are monotone.  A point the float test
// accepts has |fl(q - p)| <= sqrtf(d2) < r per axis, so |q - p| < r (1 + 2^-23)
// <= r' = r (1 + 2^-10) and, rounding being monotone, fl(q - r') <= p <=
// fl(q + r'): its cell lies in [cell(q - r'), cell(q + r')] on every axis.
//
// Wide boxes: a box of more cells than the index has buckets (its row runs
// capped at kPtsRowW cells) is not walked; the records are scanned linearly.
// Walking such a box would read at least as many records (cells * n / buckets
// on average) and its row count could overflow.  So every loop is bounded by
// the bucket count (rows), the record count (a bucket range, the linear scan)
// or k, never by a caller's float.
#pragma once

constexpr int kPtsRowBits = 10, kPtsRowW = 1 << kPtsRowBits;
constexpr uint64_t kPtsNone = ~uint64_t(0);

struct PtsIndex {
  const float4* rec;  // [nrec] {x, y, z, index}, bucket-sorted
  const int* start;   // [T + 1]
  int nrec;           // finite points
  uint32_t tmask;     // T - 1
  float org[3];
  float cell;
};

__device__ __forceinline__ bool pts_finite3(float x, float y, float z) {
  return isfinite(x) && isfinite(y) && isfinite(z);
}
__device__ __forceinline__ int pts_cell(float x, float org, float cell) {
  const float c = floorf((x - org) / cell);
  return static_cast<int>(clampv(c, -1073741824.f, 1073741824.f));
}
__device__ __forceinline__ uint32_t pts_row(int y, int z, uint32_t tmask) {
  return (((static_cast<uint32_t>(y) * 19349663u) ^ (static_cast<uint32_t>(z) * 83492791u)) << kPtsRowBits) & tmask;
}
__device__ __forceinline__ float pts_d2(float qx, float qy, float qz, float4 r) {
  const float dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
  return dx * dx + dy * dy + dz * dz;
}
// floats ordered as unsigned integers (for atomicMin)
__device__ __forceinline__ uint32_t pts_ord(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// ---- build
// bounding-box minimum of the finite points, as ordered integers in lo[3]
__global__ void __launch_bounds__(256) k_pts_bbox(const float* pos, int n, uint32_t* lo) {
  uint32_t m[3] = {~0u, ~0u, ~0u};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float x = pos[3 * size_t(i)], y = pos[3 * size_t(i) + 1], z = pos[3 * size_t(i) + 2];
    if (!pts_finite3(x, y, z)) continue;
    m[0] = min(m[0], pts_ord(x));
    m[1] = min(m[1], pts_ord(y));
    m[2] = min(m[2], pts_ord(z));
  }
  for (int a = 0; a < 3; ++a) {
    for (int s = 32; s > 0; s >>= 1) m[a] = min(m[a], static_cast<uint32_t>(__shfl_xor(static_cast<int>(m[a]), s)));
    if (__lane_id() == 0 && m[a] != ~0u) atomicMin(&lo[a], m[a]);
  }
}

// sort keys: the bucket of a finite point, T (past every bucket) for the others
__global__ void __launch_bounds__(256) k_pts_keys(const float* pos, int n, PtsIndex X, uint32_t* key, int* val) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float x = pos[3 * size_t(i)], y = pos[3 * size_t(i) + 1], z = pos[3 * size_t(i) + 2];
    uint32_t k = X.tmask + 1u;
    if (pts_finite3(x, y, z))
      k = pts_row(pts_cell(y, X.org[1], X.cell), pts_cell(z, X.org[2], X.cell), X.tmask) |
          (static_cast<uint32_t>(pts_cell(x, X.org[0], X.cell)) & (kPtsRowW - 1));
    key[i] = k;
    val[i] = i;
  }
}

// after the sort: the records, in sorted order
__global__ void __launch_bounds__(256) k_pts_records(const float* pos, int n, uint32_t T, const uint32_t* key,
                                                     const int* val, float4* rec) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    if (key[j] >= T) continue;  // the non-finite points sort last: j >= nrec
    const int i = val[j];
    rec[j] = make_float4(pos[3 * size_t(i)], pos[3 * size_t(i) + 1], pos[3 * size_t(i) + 2], __int_as_float(i));
  }
}

// start[b] = the first sorted position whose key is >= b, b = 0 .. T
__global__ void __launch_bounds__(256) k_pts_start(const uint32_t* key, int n, uint32_t T, int* start) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b <= T; b += gridDim.x * blockDim.x) {
    int lo = 0, hi = n;
    while (lo < hi) {  // at most 29 steps
      const int mid = lo + ((hi - lo) >> 1);
      if (key[mid] < b) lo = mid + 1;
      else hi = mid;
    }
    start[b] = lo;
  }
}

__global__ void __launch_bounds__(256) k_pts_max_bucket(const int* start, uint32_t T, int* out) {
  int m = 0;
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < T; b += gridDim.x * blockDim.x)
    m = max(m, start[b + 1] - start[b]);
  for (int s = 32; s > 0; s >>= 1) m = max(m, __shfl_xor(m, s));
  if (__lane_id() == 0 && m > 0) atomicMax(out, m);
}

// ---- the cells of a query box
struct PtsBox {
  int x0, x1, y0, y1, z0, z1;
  bool linear;  // more cells than buckets: scan the records instead
};
__device__ __forceinline__ PtsBox pts_box(const PtsIndex& X, float qx, float qy, float qz, float rq) {
  PtsBox b;
  b.x0 = pts_cell(qx - rq, X.org[0], X.cell), b.x1 = pts_cell(qx + rq, X.org[0], X.cell);
  b.y0 = pts_cell(qy - rq, X.org[1], X.cell), b.y1 = pts_cell(qy + rq, X.org[1], X.cell);
  b.z0 = pts_cell(qz - rq, X.org[2], X.cell), b.z1 = pts_cell(qz + rq, X.org[2], X.cell);
  // cells are within +-2^30, so each extent is at most 2^31 + 1; the product in steps that cannot overflow
  const int64_t T = int64_t(X.tmask) + 1;
  const int64_t nx = min(int64_t(b.x1) - b.x0 + 1, int64_t(kPtsRowW));
  const int64_t ny = int64_t(b.y1) - b.y0 + 1, nz = int64_t(b.z1) - b.z0 + 1;
  b.linear = ny > T || nz > T || ny * nz > T || ny * nz * nx > T;
  return b;
}

// ---- KdTree::searchInRadius, one query per lane (the measured alternative,
// see WR_PTS_RADIUS_WAVE below).  FILL = false: count[j];
// FILL = true: the indices at index[offset[j] ..], at most offset[j + 1] -
// offset[j] of them, and nothing unless 0 <= offset[j] <= offset[j + 1] <= capacity.
template <bool FILL>
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_pts_radius(PtsIndex X, const float* q, int64_t nq, float radius,
                                                                  const float* radii, const int64_t* offset,
                                                                  int64_t capacity, int32_t* count, int32_t* index) {
  for (int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < nq;
       j += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const float qx = q[3 * j], qy = q[3 * j + 1], qz = q[3 * j + 2];
    const float r = radii ? radii[j] : radius;
    int64_t o0 = 0, room = 0;
    if (FILL) {
      o0 = offset[j];
      const int64_t o1 = offset[j + 1];
      room = (o0 >= 0 && o1 >= o0 && o1 <= capacity) ? o1 - o0 : 0;
    }
    int64_t cnt = 0;
    if (pts_finite3(qx, qy, qz) && r > 0.f && (!FILL || room > 0)) {  // (r NaN or <= 0: nothing is nearer)
      const PtsBox b = pts_box(X, qx, qy, qz, r * 1.0009765625f);
      if (b.linear) {
        for (int i = 0; i < X.nrec; ++i) {
          const float4 rc = X.rec[i];
          if (!(sqrtf(pts_d2(qx, qy, qz, rc)) < r)) continue;
          if (FILL && cnt < room) index[o0 + cnt] = __float_as_int(rc.w);
          ++cnt;
        }
      } else {
        const int ny = b.y1 - b.y0 + 1, nrow = ny * (b.z1 - b.z0 + 1);  // <= T
        const bool whole = b.x1 - b.x0 >= kPtsRowW - 1;
        const uint32_t xa = static_cast<uint32_t>(b.x0) & (kPtsRowW - 1), xb = static_cast<uint32_t>(b.x1) & (kPtsRowW - 1);
        const int parts = (!whole && xa > xb) ? 2 : 1;  // 2: the row's cells wrap in cx
        for (int k = 0; k < nrow; ++k) {
          const int cy = b.y0 + k % ny, cz = b.z0 + k / ny;
          const uint32_t row = pts_row(cy, cz, X.tmask);
          for (int part = 0; part < parts; ++part) {
            uint32_t lo, hi;
            if (whole) lo = row, hi = row | (kPtsRowW - 1);
            else if (parts == 1) lo = row | xa, hi = row | xb;
            else if (part == 0) lo = row | xa, hi = row | (kPtsRowW - 1);
            else lo = row, hi = row | xb;
            const int i1 = X.start[hi + 1];
            for (int i = X.start[lo]; i < i1; ++i) {
              const float4 rc = X.rec[i];
              if (!(sqrtf(pts_d2(qx, qy, qz, rc)) < r)) continue;
              // a bucket is shared by cells: the record counts only in its own row, within this box's x cells
              const int vx = pts_cell(rc.x, X.org[0], X.cell);
              if (pts_cell(rc.y, X.org[1], X.cell) != cy || pts_cell(rc.z, X.org[2], X.cell) != cz || vx < b.x0 ||
                  vx > b.x1)
                continue;
              if (FILL && cnt < room) index[o0 + cnt] = __float_as_int(rc.w);
              ++cnt;
            }
          }
        }
      }
    }
    if (!FILL) count[j] = static_cast<int32_t>(cnt);
  }
}

// The same query with one wave per query, the records of a bucket range 64 at
// a time (ballot and popcount for the count and the list positions; the same
// lists in the same order).  This is the form the library runs: on the
// photon-like workload of scripts/points_rate.py, whose queries find from
// nothing to a hundred points, it counts 2.3 times and fills 4.3 times as fast
// as the lane form (profiles/r18/points).  -DWR_PTS_RADIUS_WAVE=0 builds the
// lane form instead.
#ifndef WR_PTS_RADIUS_WAVE
#define WR_PTS_RADIUS_WAVE 1
#endif
template <bool FILL>
__device__ __forceinline__ void pts_rw_range(const PtsIndex& X, float qx, float qy, float qz, float r, int i0, int i1,
                                             bool any, int cy, int cz, int x0, int x1, int64_t& cnt, int64_t o0,
                                             int64_t room, int32_t* index) {
  const int lane = __lane_id();
  for (int base = i0; base < i1; base += 64) {
    const int i = base + lane;
    bool ok = false;
    float4 rc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < i1) {
      rc = X.rec[i];
      ok = sqrtf(pts_d2(qx, qy, qz, rc)) < r;
      if (ok && !any) {
        const int vx = pts_cell(rc.x, X.org[0], X.cell);
        ok = pts_cell(rc.y, X.org[1], X.cell) == cy && pts_cell(rc.z, X.org[2], X.cell) == cz && vx >= x0 && vx <= x1;
      }
    }
    const uint64_t m = __ballot(ok);
    if (FILL && ok) {
      const int64_t at = cnt + __popcll(m & ((uint64_t(1) << lane) - 1));
      if (at < room) index[o0 + at] = __float_as_int(rc.w);
    }
    cnt += __popcll(m);
  }
}
template <bool FILL>
__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_pts_radius_wave(PtsIndex X, const float* q, int64_t nq,
                                                                       float radius, const float* radii,
                                                                       const int64_t* offset, int64_t capacity,
                                                                       int32_t* count, int32_t* index) {
  const int64_t wave0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  for (int64_t j = wave0; j < nq; j += nwaves) {
    const float qx = q[3 * j], qy = q[3 * j + 1], qz = q[3 * j + 2];
    const float r = radii ? radii[j] : radius;
    int64_t o0 = 0, room = 0;
    if (FILL) {
      o0 = offset[j];
      const int64_t o1 = offset[j + 1];
      room = (o0 >= 0 && o1 >= o0 && o1 <= capacity) ? o1 - o0 : 0;
    }
    int64_t cnt = 0;
    if (pts_finite3(qx, qy, qz) && r > 0.f && (!FILL || room > 0)) {
      const PtsBox b = pts_box(X, qx, qy, qz, r * 1.0009765625f);
      if (b.linear) {
        pts_rw_range<FILL>(X, qx, qy, qz, r, 0, X.nrec, true, 0, 0, 0, 0, cnt, o0, room, index);
      } else {
        const int ny = b.y1 - b.y0 + 1, nrow = ny * (b.z1 - b.z0 + 1);
        const bool whole = b.x1 - b.x0 >= kPtsRowW - 1;
        const uint32_t xa = static_cast<uint32_t>(b.x0) & (kPtsRowW - 1), xb = static_cast<uint32_t>(b.x1) & (kPtsRowW - 1);
        const int parts = (!whole && xa > xb) ? 2 : 1;
        for (int k = 0; k < nrow; ++k) {
          const int cy = b.y0 + k % ny, cz = b.z0 + k / ny;
          const uint32_t row = pts_row(cy, cz, X.tmask);
          for (int part = 0; part < parts; ++part) {
            uint32_t lo, hi;
            if (whole) lo = row, hi = row | (kPtsRowW - 1);
            else if (parts == 1) lo = row | xa, hi = row | xb;
            else if (part == 0) lo = row | xa, hi = row | (kPtsRowW - 1);
            else lo = row, hi = row | xb;
            pts_rw_range<FILL>(X, qx, qy, qz, r, X.start[lo], X.start[hi + 1], false, cy, cz, b.x0, b.x1, cnt, o0, room,
                               index);
          }
        }
      }
    }
    if (!FILL && __lane_id() == 0) count[j] = static_cast<int32_t>(cnt);
  }
}

// ---- KdTree::searchKnn, one query per wave.  The best k keys (d2 bits << 32 |
// index: ordered as (d2, index), d2 >= 0) live one per lane, ascending in
// lanes 0 .. k - 1; `bound` is the smaller of the k-th key and max_sqr_dist's,
// and only keys below it enter (searchKnn shrinking maxSqrDis).  The wave reads
// 64 candidate records at a time; those below the bound are inserted one by
// one (ballot for the position, a shift by one lane).
struct PtsKnn {
  uint64_t key;    // this lane's entry
  uint64_t bound;  // wave-uniform
  uint64_t limit;  // max_sqr_dist's key, wave-uniform
  int k, lane;
};
__device__ __forceinline__ void pts_knn_offer(PtsKnn& S, uint64_t cand) {
  uint64_t m = __ballot(cand < S.bound);
  while (m) {  // at most 64 rounds
    const int src = __ffsll(static_cast<unsigned long long>(m)) - 1;
    m &= m - 1;
    const uint64_t c = __shfl(static_cast<unsigned long long>(cand), src);
    if (c >= S.bound) continue;  // the bound shrank meanwhile
    const int pos = __popcll(__ballot(S.key < c));  // < k: c is below the k-th key
    const uint64_t up = __shfl_up(static_cast<unsigned long long>(S.key), 1);
    if (S.lane == pos) S.key = c;
    else if (S.lane > pos) S.key = up;
    if (S.lane >= S.k) S.key = kPtsNone;
    const uint64_t kth = __shfl(static_cast<unsigned long long>(S.key), S.k - 1);
    S.bound = kth < S.limit ? kth : S.limit;
  }
}
// the records [i0, i1) 64 at a time; own: the cell a record must lie in (cy, cz, x in [xa, xb]), or any
__device__ __forceinline__ void pts_knn_range(PtsKnn& S, const PtsIndex& X, float qx, float qy, float qz, int i0, int i1,
                                              bool any, int cy, int cz, int xa, int xb) {
  for (int base = i0; base < i1; base += 64) {
    const int i = base + S.lane;
    uint64_t cand = kPtsNone;
    if (i < i1) {
      const float4 rc = X.rec[i];
      const float d2 = pts_d2(qx, qy, qz, rc);
      bool ok = d2 >= 0.f;  // (not NaN: inf - inf of an overflowed difference)
      if (ok && !any) {
        const int vx = pts_cell(rc.x, X.org[0], X.cell);
        ok = pts_cell(rc.y, X.org[1], X.cell) == cy && pts_cell(rc.z, X.org[2], X.cell) == cz && vx >= xa && vx <= xb;
      }
      if (ok) cand = (static_cast<uint64_t>(__float_as_uint(d2)) << 32) | static_cast<uint32_t>(__float_as_int(rc.w));
    }
    pts_knn_offer(S, cand);
  }
}
// the cells [xa, xb] of row (cy, cz): one bucket range, two where cx wraps (xb - xa < kPtsRowW - 1 here)
__device__ __forceinline__ void pts_knn_run(PtsKnn& S, const PtsIndex& X, float qx, float qy, float qz, int cy, int cz,
                                            int xa, int xb) {
  const uint32_t row = pts_row(cy, cz, X.tmask);
  const uint32_t a = static_cast<uint32_t>(xa) & (kPtsRowW - 1), b = static_cast<uint32_t>(xb) & (kPtsRowW - 1);
  if (a <= b) {
    pts_knn_range(S, X, qx, qy, qz, X.start[row | a], X.start[(row | b) + 1], false, cy, cz, xa, xb);
  } else {
    pts_knn_range(S, X, qx, qy, qz, X.start[row | a], X.start[(row | (kPtsRowW - 1)) + 1], false, cy, cz, xa, xb);
    pts_knn_range(S, X, qx, qy, qz, X.start[row], X.start[(row | b) + 1], false, cy, cz, xa, xb);
  }
}

// The search of one query by its wave: on return S holds the winners, ascending
// in lanes 0 .. (their number) - 1.  The caller has set S (k, lane, limit, bound
// = limit, key = none) and checked that the query is finite and the limit > 0.
__device__ __forceinline__ void pts_knn_search(PtsKnn& S, const PtsIndex& X, float qx, float qy, float qz) {
  const int64_t T = int64_t(X.tmask) + 1;
  const int cx = pts_cell(qx, X.org[0], X.cell), cy = pts_cell(qy, X.org[1], X.cell),
            cz = pts_cell(qz, X.org[2], X.cell);
  // Before shell s is read, the box of shell s - 1 has been.  A record
  // outside it lies s or more cells from the query's cell on some axis, so
  // (the query being anywhere in its cell) more than s - 1 - err cell
  // edges away, err bounding the rounding of the two cell computations
  // (2^-20 of the coordinates in cells); with the margin of r', every
  // such record has d2 >= lb^2 (1 - 2^-9).
  const float cmax = fmaxf(fmaxf(fabsf(static_cast<float>(cx)), fabsf(static_cast<float>(cy))),
                           fabsf(static_cast<float>(cz)));
  bool linear = false;
  for (int s = 0;; ++s) {  // (2 s + 1)^3 <= T: s < 2^10
    const int64_t w = 2 * int64_t(s) + 1;
    if (w * w * w > T) {
      linear = true;
      break;
    }
    if (s > 1) {
      const float lbc = static_cast<float>(s - 1) - (cmax + static_cast<float>(s) + 2.f) * 9.5367431640625e-7f;
      const float lb = lbc * X.cell * 0.9990234375f;
      const float bd2 = __uint_as_float(static_cast<uint32_t>(S.bound >> 32));
      if (lbc > 0.f && lb * lb * 0.998046875f > bd2) break;  // nothing out there is below the bound
    }
    for (int dz = -s; dz <= s; ++dz)
      for (int dy = -s; dy <= s; ++dy) {
        if (max(abs(dy), abs(dz)) == s) {
          pts_knn_run(S, X, qx, qy, qz, cy + dy, cz + dz, cx - s, cx + s);
        } else {  // an inner row: its two end cells belong to this shell
          pts_knn_run(S, X, qx, qy, qz, cy + dy, cz + dz, cx - s, cx - s);
          pts_knn_run(S, X, qx, qy, qz, cy + dy, cz + dz, cx + s, cx + s);
        }
      }
  }
  if (linear) {  // the shells outgrew the buckets: start over, every record once
    S.key = kPtsNone;
    S.bound = S.limit;
    pts_knn_range(S, X, qx, qy, qz, 0, X.nrec, true, 0, 0, 0, 0);
  }
}

__global__ void __launch_bounds__(256) WR_NO_PK_FP32 k_pts_knn(PtsIndex X, const float* q, int64_t nq, int k,
                                                               float max_sqr_dist, int32_t* index, float* sqr_dist,
                                                               int32_t* count) {
  const int lane = __lane_id();
  const int64_t wave0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  for (int64_t j = wave0; j < nq; j += nwaves) {
    const float qx = q[3 * j], qy = q[3 * j + 1], qz = q[3 * j + 2];
    PtsKnn S;
    S.k = k, S.lane = lane;
    S.key = kPtsNone;
    S.limit = static_cast<uint64_t>(__float_as_uint(max_sqr_dist)) << 32;  // d2 < max_sqr_dist, strictly
    S.bound = S.limit;
    if (pts_finite3(qx, qy, qz) && max_sqr_dist > 0.f) pts_knn_search(S, X, qx, qy, qz);
    const bool have = S.key != kPtsNone;
    if (lane < k) {
      index[j * k + lane] = have ? static_cast<int32_t>(static_cast<uint32_t>(S.key)) : -1;
      sqr_dist[j * k + lane] = have ? __uint_as_float(static_cast<uint32_t>(S.key >> 32)) : 0.f;
    }
    const int found = __popcll(__ballot(have));
    if (lane == 0) count[j] = found;
  }
}
