// gwi_popdraw.h -- fair draws from tabulated 1-D densities: the inverse CDF of a piecewise-linear curve, inverted exactly
// (include/gwi_engine.h: gwi_table_draws; the NumPy statement is gwinferno_amd/population_draws.py).
//
// A table is an unnormalised density p[0..G) on the uniform grid lo ... hi, read as piecewise linear -- the reading the trapezoid
// curves of postprocess.py make.  Cell c = [x_c, x_{c+1}] has mass m_c = (p_c + p_{c+1}) dx / 2 and C_c is the inclusive prefix.
//
//   table_cdf_kernel   one workgroup per table: the G - 1 cell masses and their inclusive prefix into HBM -- a block scan in
//                      chunks of 256 with a carry, as draw_merge_kernel does -- and the last cell with mass.  No atomics: the
//                      prefix of a table is the same bits on every launch.
//   table_draw_kernel  grid = (blocks of draws, tables), lane = draw.  The workgroup stages its table's prefix and density in
//                      LDS (dynamic: (2 G - 1) doubles, 24 KB at the reference's largest grid of 1 500 points).  Draw j of
//                      table t takes ONE Philox4x32-10 block -- counter (index low, index high, t, kTag), index = first_index + j,
//                      key = the seed's halves -- for the two uniforms u (the draw) and v (the thinning decision).  A binary
//                      search finds a cell whose prefix exceeds the target u C_last; the parallel prefix is not monotone to the
//                      last bit, so gwi_draw.h's two rules hold here too: a cell without mass is never chosen (the search
//                      result moves on to the next cell with mass), and a target past the end takes the last cell with mass.
//                      Inside the cell the residual mass r is inverted in the cancellation-free form
//                          x = x_c + 2 r / (p_c + sqrt(p_c^2 + 2 s r)),   s = (p_{c+1} - p_c) / dx,
//                      exact for s = 0 and well defined for p_c = 0; the result is clamped into the cell.
//                      With a per-draw lower bound the draw comes from the density restricted to x >= lower: C(lower) = the
//                      prefix up to lower's cell + that cell's partial trapezoid, target = C(lower) + u (C_last - C(lower)),
//                      mass = 1 - C(lower) / C_last (the probability the restriction keeps) and accept = (v < mass).
//                      lower <= lo is no bound (mass 1, accept 1); with no mass at or above lower: x = min(max(lower, lo), hi),
//                      mass 0, accept 0; a NaN bound gives NaN, NaN, 0.
//
// Plain vector loads and stores, no scratch, no log / exp; sqrt is the device library's; contraction is off wherever a value is
// formed that the NumPy statement forms too.  Every loop is bounded by the number of cells.
#pragma once

#include <hip/hip_runtime.h>

#include "gwi_draw.h"
#include "gwi_spinprior.h"

namespace gwi {
namespace popdraw {

constexpr int kBlock = draw::kDrawBlock;  // the block scan and reduction of gwi_draw.h are written for it
constexpr int kMaxGrid = 4096;            // prefix + density of one table in LDS: at most 64 KB
constexpr unsigned kTag = 0x504F5044u;    // counter word 3; the chi_p kernel's is 2 * attempt (+ 1) < 2^17

__device__ inline double cell_mass(double p0, double p1, double dx) {
#pragma clang fp contract(off)
  return 0.5 * (p0 + p1) * dx;
}

struct CdfArgs {
  const double *pdf, *lo, *hi;  // [n_tables][n_grid], [n_tables], [n_tables]
  double* prefix;               // [n_tables][n_grid - 1]
  int* last_live;               // [n_tables]: the last cell with mass, -1 for none
  int n_grid;
};

__global__ __launch_bounds__(kBlock) void table_cdf_kernel(const CdfArgs a) {
#pragma clang fp contract(off)
  __shared__ double lds[kBlock / 64];
  __shared__ int ldi[kBlock / 64];
  const int t = blockIdx.x, n_cell = a.n_grid - 1;
  const double* p = a.pdf + (long long)t * a.n_grid;
  double* out = a.prefix + (long long)t * n_cell;
  const double dx = (a.hi[t] - a.lo[t]) / (double)n_cell;
  double carry = 0.0;
  int live = -1;
  for (int base = 0; base < n_cell; base += kBlock) {  // (the trip count is the same for every thread)
    const int c = base + (int)threadIdx.x;
    const double m = c < n_cell ? cell_mass(p[c], p[c + 1], dx) : 0.0;
    if (m > 0.0) live = c;
    double total;
    const double incl = draw::block_inclusive_scan(m, lds, &total);
    if (c < n_cell) out[c] = carry + incl;
    carry += total;
  }
  live = draw::block_reduce(live, ldi, draw::OpMax());
  if (threadIdx.x == 0) a.last_live[t] = live;
}

struct DrawArgs {
  const double *pdf, *lo, *hi, *prefix;  // of every table of the call
  const int* last_live;
  const double* lower;                   // [tables of this launch][ld] or null
  double* x;                             // [tables of this launch][ld]
  double* mass;                          // or null
  unsigned char* accept;                 // or null
  unsigned long long seed, first_index;  // first_index: the stream index of this launch's draw 0
  long long n_draws, ld;                 // draws per table in this launch; row stride of the launch's buffers
  int n_grid, first_table;               // first_table: the table of blockIdx.y == 0
};

struct Drawn {
  double x, mass;
  unsigned char accept;
};

// one draw from the table staged at (prefix sC[n_cell], density sP[n_cell + 1])
__device__ inline Drawn draw_one(const double* sC, const double* sP, int n_cell, int last_live, double lo, double hi, double dx, bool has_lower, double lw, double u,
                                 double v) {
#pragma clang fp contract(off)
  const double c_last = sC[n_cell - 1];
  if (last_live < 0) return Drawn{__builtin_nan(""), 0.0, 0};  // (the entry point refuses a table without mass)
  int c_min = 0;
  double c_low = 0.0, mass = 1.0;
  bool bounded = false;
  if (has_lower) {
    if (!(lw == lw)) return Drawn{lw, lw, 0};
    if (lw > lo) {
      bounded = true;
      bool empty = lw > hi;
      if (!empty) {
        int cl = (int)((lw - lo) / dx);
        if (cl > n_cell - 1) cl = n_cell - 1;
        if (lw < lo + (double)cl * dx) cl -= 1;  // (the quotient rounded up; cl >= 1 here, since lw > lo)
        const double d = fmin(fmax(lw - (lo + (double)cl * dx), 0.0), dx);
        const double p0 = sP[cl], p1 = sP[cl + 1], s = (p1 - p0) / dx, m = cell_mass(p0, p1, dx);
        const double part = fmin(fmax(d * (p0 + 0.5 * s * d), 0.0), m);  // the trapezoid from x_cl to lower
        if (cl > last_live || (cl == last_live && !(part < m))) {
          empty = true;
        } else {
          c_min = cl;
          c_low = (cl > 0 ? sC[cl - 1] : 0.0) + part;
          if (!(c_last - c_low > 0.0)) empty = true;
        }
      }
      if (empty) return Drawn{fmin(fmax(lw, lo), hi), 0.0, 0};
      mass = fmin(fmax(1.0 - c_low / c_last, 0.0), 1.0);
    }
  }
  const double target = bounded ? c_low + u * (c_last - c_low) : u * c_last;
  // a cell in [c_min, n_cell) whose prefix exceeds the target while its predecessor's does not
  int a = c_min, b = n_cell;
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (sC[mid] > target) b = mid;
    else a = mid + 1;
  }
  int c = a;
  while (c < n_cell && !(cell_mass(sP[c], sP[c + 1], dx) > 0.0)) ++c;  // never a cell without mass
  if (c >= n_cell) c = last_live;                                      // past the end: the last cell with mass (>= c_min)
  const double p0 = sP[c], p1 = sP[c + 1], s = (p1 - p0) / dx, m = cell_mass(p0, p1, dx);
  const double r = fmin(fmax(target - (c > 0 ? sC[c - 1] : 0.0), 0.0), m);
  const double den = p0 + sqrt(fmax(p0 * p0 + 2.0 * s * r, 0.0));
  const double xc = lo + (double)c * dx, xr = c + 1 == n_cell ? hi : lo + (double)(c + 1) * dx;
  double x = den > 0.0 ? xc + 2.0 * r / den : xc;
  x = fmin(fmax(x, xc), xr);
  if (bounded) x = fmax(x, lw);
  return Drawn{x, mass, (unsigned char)(v < mass ? 1 : 0)};
}

__global__ __launch_bounds__(kBlock) void table_draw_kernel(const DrawArgs a) {
  extern __shared__ double popdraw_lds[];
  const int n_cell = a.n_grid - 1, row = blockIdx.y, t = a.first_table + row;
  double* sC = popdraw_lds;
  double* sP = popdraw_lds + n_cell;
  const double* gC = a.prefix + (long long)t * n_cell;
  const double* gP = a.pdf + (long long)t * a.n_grid;
  for (int i = threadIdx.x; i < n_cell; i += kBlock) sC[i] = gC[i];
  for (int i = threadIdx.x; i < a.n_grid; i += kBlock) sP[i] = gP[i];
  __syncthreads();
  const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (j >= a.n_draws) return;  // (no barrier below)
  const double lo = a.lo[t], hi = a.hi[t], dx = (hi - lo) / (double)n_cell;
  const unsigned long long index = a.first_index + (unsigned long long)j;
  const spinprior::U4 w = spinprior::philox4x32_10(spinprior::U4{(unsigned)index, (unsigned)(index >> 32), (unsigned)t, kTag}, (unsigned)a.seed, (unsigned)(a.seed >> 32));
  const long long at = (long long)row * a.ld + j;
  const Drawn d = draw_one(sC, sP, n_cell, a.last_live[t], lo, hi, dx, a.lower != nullptr, a.lower ? a.lower[at] : 0.0, spinprior::uniform53(w.x, w.y),
                           spinprior::uniform53(w.z, w.w));
  a.x[at] = d.x;
  if (a.mass) a.mass[at] = d.mass;
  if (a.accept) a.accept[at] = d.accept;
}

}  // namespace popdraw
}  // namespace gwi
