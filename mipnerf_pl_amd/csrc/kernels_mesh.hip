// Geometry out of a trained field (gfx950, wave64), compiled with -ffp-contract=off:
//   k_lattice_ipe / k_store_sigma   the encoding rows of a lattice of isotropic Gaussians straight from the lattice index, in front of
//                                   the MLP kernels, and the activated density behind them;
//   k_iso_*                         marching tetrahedra on the Kuhn split of any fp32 lattice [nz, ny, nx]: classify (one sign bit and one
//                                   7-bit edge mask per lattice point, kept in the workspace), two exclusive scans (vertices per point,
//                                   faces per cell; sums per 1024 points + one single-workgroup scan + per-point bases, no atomics: two
//                                   runs give the same bytes), emit (vertex index = base[point] + popcount(mask[point] & below(slot))).
// Everything is HBM-bound elementwise / gather work: lattice reads are coalesced along x, every result leaves through ordinary
// vector stores.
#include <hip/hip_runtime.h>

#include "ipe.hpp"
#include "kernels.hpp"
#include "lane_buckets.hpp"
#include "lattice.hpp"
#include "raymath.hpp"

namespace mip {

// Two threads per lattice point, as k_integrated_pos_enc: no means or covariances go through memory.
template <typename OutT, int L>
__global__ void __launch_bounds__(256)
k_lattice_ipe(Lattice g, int64_t first, int64_t count, float cov_scale, int min_deg, OutT* __restrict__ enc) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t s = gid >> 1;
    const int q = (int)(gid & 1);
    if (s >= count) return;
    int idx[3];
    lattice_ijk(g, (int)(first + s), idx[0], idx[1], idx[2]);
    Gauss3 gs;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float h = lattice_step(g, a);
        gs.mean[a] = g.lo[a] + (float)idx[a] * h;
        gs.cov[a] = cov_scale * h * h / 12.0f;      // variance of a uniform box of side h
    }
    ipe_write<OutT, L>(gs, q, min_deg, enc + s * (int64_t)(6 * L));
}

__global__ void __launch_bounds__(256)
k_store_sigma(int64_t count, const float4* __restrict__ rgb_sigma, float* __restrict__ sigma) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < count) sigma[s] = rgb_sigma[s].w;
}

hipError_t launch_lattice_ipe(const int dims[3], const float lo[3], const float hi[3], int64_t first, int64_t count, float cov_scale,
                              int min_deg, int max_deg, void* enc, bool bf16, hipStream_t st) {
    if (max_deg - min_deg != 16) return hipErrorInvalidValue;   // generated for L = 16, as the ray-side encoders
    Lattice g;
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2];
    for (int a = 0; a < 3; ++a) { g.lo[a] = lo[a]; g.hi[a] = hi[a]; }
    const int64_t threads = 2 * count;
    if (bf16)
        hipLaunchKernelGGL((k_lattice_ipe<__bf16, 16>), dim3(grid_for(threads, 256)), dim3(256), 0, st, g, first, count, cov_scale,
                           min_deg, (__bf16*)enc);
    else
        hipLaunchKernelGGL((k_lattice_ipe<float, 16>), dim3(grid_for(threads, 256)), dim3(256), 0, st, g, first, count, cov_scale,
                           min_deg, (float*)enc);
    return hipGetLastError();
}

hipError_t launch_store_sigma(int64_t count, const float* rgb_sigma, float* sigma, hipStream_t st) {
    hipLaunchKernelGGL(k_store_sigma, dim3(grid_for(count, 256)), dim3(256), 0, st, count, (const float4*)rgb_sigma, sigma);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// marching tetrahedra, Kuhn split
// ------------------------------------------------------------------------------------------
// A cell corner is the 3-bit code dx + 2 dy + 4 dz; edge slot s of a lattice point leads to the neighbour with the code s + 1
// (x, y, xy, z, xz, yz, xyz: the order of the far end's flat index).  Tetrahedron p (the permutations of the axes in lexicographic
// order) has the corners (0, e_p0, e_p0 + e_p1, 7); their codes increase, so does their flat index.
//
// The table below is DERIVED, not typed: for every tetrahedron and every one of the 16 sign cases (bit v = corner v inside) it holds up to
// two triangles; a triangle corner is the crossed edge (m, n), m < n corner numbers of the tetrahedron, stored as (cell corner code of
// m) | (slot << 3) with slot = code(n) - code(m) - 1.  Winding: normal from inside to outside, from the sign case and the orientation of
// the tetrahedron alone -- the winding the triangle through the three edge midpoints has:
//   one corner a apart from the other three o0 < o1 < o2: det[o0 - a, o1 - a, o2 - a] = (-1)^a sign(p); (a o0, a o1, a o2) looks away
//     from a when that is positive; a is the lone INSIDE corner: keep it then, a is the lone OUTSIDE corner: reverse it then;
//   two inside a0 < a1, two outside o0 < o1: the quad (a0 o0, a0 o1, a1 o1, a1 o0), cut along its first diagonal, looks from a0 to o0
//     when det[a1 - a0, o0 - a0, o1 - a0] = parity(a0 a1 o0 o1) sign(p) is positive.
struct TetTable {
    unsigned char code1[6], code2[6];       // cell corner codes of the tetrahedron's corners 1 and 2 (corner 0 is 0, corner 3 is 7)
    unsigned char ntri[6][16];
    unsigned char edge[6][16][2][3];
};

constexpr int kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
constexpr int kPermSign[6] = {1, -1, -1, 1, 1, -1};

constexpr unsigned char tet_edge(const int code[4], int u, int v) {      // the edge between corners u and v of a tetrahedron
    const int m = u < v ? u : v, n = u < v ? v : u;
    return (unsigned char)(code[m] | ((code[n] - code[m] - 1) << 3));
}

constexpr TetTable make_tet_table() {
    TetTable t = {};
    for (int p = 0; p < 6; ++p) {
        const int code[4] = {0, 1 << kPerm[p][0], (1 << kPerm[p][0]) | (1 << kPerm[p][1]), 7};
        t.code1[p] = (unsigned char)code[1];
        t.code2[p] = (unsigned char)code[2];
        for (int c = 0; c < 16; ++c) {
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
            for (int v = 0; v < 4; ++v) {
                if ((c >> v) & 1) in[ni++] = v; else out[no++] = v;
            }
            if (ni == 0 || ni == 4) continue;
            if (ni == 2) {
                // parity of the permutation (a0, a1, o0, o1) of (0, 1, 2, 3): count inversions
                const int seq[4] = {in[0], in[1], out[0], out[1]};
                int inv = 0;
                for (int x = 0; x < 4; ++x)
                    for (int y = x + 1; y < 4; ++y) inv += seq[x] > seq[y];
                const bool keep = ((inv & 1) ? -1 : 1) * kPermSign[p] > 0;
                const unsigned char q0 = tet_edge(code, in[0], out[0]), q1 = tet_edge(code, in[0], out[1]);
                const unsigned char q2 = tet_edge(code, in[1], out[1]), q3 = tet_edge(code, in[1], out[0]);
                t.ntri[p][c] = 2;
                t.edge[p][c][0][0] = q0; t.edge[p][c][0][1] = keep ? q1 : q2; t.edge[p][c][0][2] = keep ? q2 : q1;
                t.edge[p][c][1][0] = q0; t.edge[p][c][1][1] = keep ? q2 : q3; t.edge[p][c][1][2] = keep ? q3 : q2;
            } else {
                const int a = ni == 1 ? in[0] : out[0];
                const int* o = ni == 1 ? out : in;
                const bool away = ((a & 1) ? -1 : 1) * kPermSign[p] > 0;       // (a o0, a o1, a o2) looks away from a
                const bool keep = ni == 1 ? away : !away;
                t.ntri[p][c] = 1;
                t.edge[p][c][0][0] = tet_edge(code, a, o[0]);
                t.edge[p][c][0][1] = tet_edge(code, a, keep ? o[1] : o[2]);
                t.edge[p][c][0][2] = tet_edge(code, a, keep ? o[2] : o[1]);
            }
        }
    }
    return t;
}

__constant__ TetTable c_tet = make_tet_table();

constexpr int kIsoBlock = 256;          // threads of a workgroup of the per-point passes
constexpr int kIsoPer = 4;              // consecutive lattice points per thread: one uchar4 of masks, one uint4 of bases
constexpr int kIsoTile = kIsoBlock * kIsoPer;
constexpr int kIsoScanBlock = 1024;     // the one workgroup of the top-level scan, kIsoPer block sums per thread and iteration

struct IsoGrid {
    int nx, ny, nz;
    int n;            // nx * ny * nz (7 n < 2^31, checked by the caller)
};

__device__ __forceinline__ int iso_offset(const IsoGrid& g, int code) {      // flat index distance to the neighbour with that corner code
    return (code & 1) + ((code >> 1) & 1) * g.nx + ((code >> 2) & 1) * g.nx * g.ny;
}

// the 8 corner signs of the cell whose first corner has this mask byte (bit 7: inside; bit s: the sign differs across edge slot s)
__device__ __forceinline__ unsigned iso_cell_corners(unsigned m) {
    // bit c of the result = corner c inside; corner 0 is the point itself, corner c = slot c - 1
    const unsigned self = (m >> 7) & 1u;
    const unsigned diff = (m & 0x7fu) << 1;
    return ((self ? ~diff : diff) & 0xfeu) | self;
}

__device__ __forceinline__ unsigned iso_tet_case(unsigned corners, int p) {
    const int c1 = c_tet.code1[p], c2 = c_tet.code2[p];
    return (corners & 1u) | (((corners >> c1) & 1u) << 1) | (((corners >> c2) & 1u) << 2) | (((corners >> 7) & 1u) << 3);
}

__device__ __forceinline__ unsigned iso_cell_faces(unsigned corners) {
    unsigned nf = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p) nf += c_tet.ntri[p][iso_tet_case(corners, p)];
    return nf;
}

// Workgroup-wide exclusive scans of two values per thread at once (WAVES * 64 threads; s_wave holds 2 * WAVES words): a and b become
// their exclusive prefixes, ta / tb the workgroup's sums.  Fixed order: the same inputs give the same outputs.
template <int WAVES>
__device__ __forceinline__ void iso_block_scan2(unsigned& a, unsigned& b, unsigned* s_wave, unsigned& ta, unsigned& tb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned ia = a, ib = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned oa = __shfl_up(ia, d, 64), ob = __shfl_up(ib, d, 64);
        if (lane >= d) { ia += oa; ib += ob; }
    }
    __syncthreads();                      // s_wave may still be read by an earlier call
    if (lane == 63) { s_wave[wave] = ia; s_wave[WAVES + wave] = ib; }
    __syncthreads();
    unsigned base_a = 0, base_b = 0;
    ta = tb = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const unsigned xa = s_wave[w], xb = s_wave[WAVES + w];
        if (w < wave) { base_a += xa; base_b += xb; }
        ta += xa;
        tb += xb;
    }
    a = base_a + ia - a;
    b = base_b + ib - b;
}

// pass 1: kIsoPer consecutive lattice points per thread; mask bytes + the workgroup's vertex and face counts
__global__ void __launch_bounds__(kIsoBlock)
k_iso_classify(IsoGrid g, const float* __restrict__ f, float thr, unsigned char* __restrict__ mask, unsigned* __restrict__ block_v,
               unsigned* __restrict__ block_f) {
    __shared__ unsigned s_wave[2 * kIsoBlock / 64];
    const int p0 = (blockIdx.x * kIsoBlock + threadIdx.x) * kIsoPer;
    unsigned nv = 0, nf = 0, packed = 0;
    if (p0 < g.n) {
        const int row = p0 / g.nx;
        int i = p0 - row * g.nx, k = row / g.ny, j = row - k * g.ny;
#pragma unroll
        for (int r = 0; r < kIsoPer; ++r) {
            const int p = p0 + r;
            if (p >= g.n) break;
            const bool in = f[p] > thr;                                   // NaN and a value equal to the threshold are outside
            const bool ex = i + 1 < g.nx, ey = j + 1 < g.ny, ez = k + 1 < g.nz;
            unsigned m = 0;
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                const int code = s + 1;
                const bool there = (!(code & 1) || ex) && (!(code & 2) || ey) && (!(code & 4) || ez);
                if (there && ((f[p + iso_offset(g, code)] > thr) != in)) m |= 1u << s;
            }
            nv += __popc(m);
            if (in) m |= 0x80u;
            if (ex && ey && ez) nf += iso_cell_faces(iso_cell_corners(m));
            packed |= m << (8 * r);
            if (++i == g.nx) { i = 0; if (++j == g.ny) { j = 0; ++k; } }
        }
        if (p0 + kIsoPer <= g.n) {
            *reinterpret_cast<unsigned*>(mask + p0) = packed;            // p0 is a multiple of 4 and the mask array 16-byte aligned
        } else {
            for (int r = 0; p0 + r < g.n; ++r) mask[p0 + r] = (unsigned char)(packed >> (8 * r));
        }
    }
    unsigned tv, tf;
    iso_block_scan2<kIsoBlock / 64>(nv, nf, s_wave, tv, tf);
    if (threadIdx.x == 0) { block_v[blockIdx.x] = tv; block_f[blockIdx.x] = tf; }
}

// pass 2: ONE workgroup turns the block sums into exclusive block bases in place, in index order; totals[0] = V, totals[1] = F
__global__ void __launch_bounds__(kIsoScanBlock)
k_iso_scan_blocks(int nblocks, unsigned* __restrict__ block_v, unsigned* __restrict__ block_f, unsigned* __restrict__ totals) {
    __shared__ unsigned s_wave[2 * kIsoScanBlock / 64];
    unsigned run_v = 0, run_f = 0;
    for (int b0 = 0; b0 < nblocks; b0 += kIsoScanBlock * kIsoPer) {
        const int b = b0 + threadIdx.x * kIsoPer;
        unsigned v[kIsoPer], fc[kIsoPer], sv = 0, sf = 0;
#pragma unroll
        for (int r = 0; r < kIsoPer; ++r) {
            v[r] = b + r < nblocks ? block_v[b + r] : 0u;
            fc[r] = b + r < nblocks ? block_f[b + r] : 0u;
            sv += v[r];
            sf += fc[r];
        }
        unsigned tv, tf;
        iso_block_scan2<kIsoScanBlock / 64>(sv, sf, s_wave, tv, tf);
#pragma unroll
        for (int r = 0; r < kIsoPer; ++r) {
            if (b + r < nblocks) { block_v[b + r] = run_v + sv; block_f[b + r] = run_f + sf; }
            sv += v[r];
            sf += fc[r];
        }
        run_v += tv;
        run_f += tf;
    }
    if (threadIdx.x == 0) { totals[0] = run_v; totals[1] = run_f; }
}

// pass 3: the index of every point's first vertex
__global__ void __launch_bounds__(kIsoBlock)
k_iso_bases(IsoGrid g, const unsigned char* __restrict__ mask, const unsigned* __restrict__ block_v, unsigned* __restrict__ vbase) {
    __shared__ unsigned s_wave[2 * kIsoBlock / 64];
    const int p0 = (blockIdx.x * kIsoBlock + threadIdx.x) * kIsoPer;
    unsigned cnt[kIsoPer] = {0, 0, 0, 0}, nv = 0, unused = 0;
    if (p0 + kIsoPer <= g.n) {
        const unsigned packed = *reinterpret_cast<const unsigned*>(mask + p0);
#pragma unroll
        for (int r = 0; r < kIsoPer; ++r) cnt[r] = __popc((packed >> (8 * r)) & 0x7fu);
    } else {
        for (int r = 0; p0 + r < g.n; ++r) cnt[r] = __popc(mask[p0 + r] & 0x7fu);
    }
#pragma unroll
    for (int r = 0; r < kIsoPer; ++r) nv += cnt[r];
    unsigned tv, tu;
    iso_block_scan2<kIsoBlock / 64>(nv, unused, s_wave, tv, tu);
    unsigned run = block_v[blockIdx.x] + nv;
    for (int r = 0; r < kIsoPer && p0 + r < g.n; ++r) {
        vbase[p0 + r] = run;
        run += cnt[r];
    }
}

// grad f at a lattice point: central differences, one-sided on the faces of the box
__device__ __forceinline__ void iso_gradient(const IsoGrid& g, const float* __restrict__ f, int p, int i, int j, int k, const float h[3],
                                             float out[3]) {
    const int idx[3] = {i, j, k}, n[3] = {g.nx, g.ny, g.nz}, st[3] = {1, g.nx, g.nx * g.ny};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int up = idx[a] + 1 < n[a] ? st[a] : 0, dn = idx[a] > 0 ? st[a] : 0;
        const float span = (up && dn) ? 2.0f * h[a] : h[a];
        out[a] = (f[p + up] - f[p - dn]) / span;
    }
}

// the vertices of lattice point p = (i, j, k) with mask byte m, written from index v on
__device__ __forceinline__ void iso_emit_vertices(const IsoGrid& g, const Lattice& box, const float* __restrict__ f, float thr, int p, int i,
                                                  int j, int k, unsigned m, unsigned v, float* __restrict__ vertices,
                                                  float* __restrict__ normals, long long* __restrict__ vertex_edges) {
    const float h[3] = {lattice_step(box, 0), lattice_step(box, 1), lattice_step(box, 2)};
    const bool in = (m & 0x80u) != 0;
    const float fp = f[p];
    const float pp[3] = {box.lo[0] + (float)i * h[0], box.lo[1] + (float)j * h[1], box.lo[2] + (float)k * h[2]};
    float gp[3] = {0.f, 0.f, 0.f};
    if (normals) iso_gradient(g, f, p, i, j, k, h, gp);
    for (int s = 0; s < 7; ++s) {
        if (!((m >> s) & 1u)) continue;
        const int code = s + 1, q = p + iso_offset(g, code);
        const int qi = i + (code & 1), qj = j + ((code >> 1) & 1), qk = k + ((code >> 2) & 1);
        const float fq = f[q];
        const float pq[3] = {box.lo[0] + (float)qi * h[0], box.lo[1] + (float)qj * h[1], box.lo[2] + (float)qk * h[2]};
        const float f_in = in ? fp : fq, f_out = in ? fq : fp;
        float t = (thr - f_in) / (f_out - f_in);
        if (!(fabsf(t) <= 3.402823466e38f)) t = 0.5f;                    // an end is infinite or NaN: positions stay finite
        if (vertices) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float x_in = in ? pp[a] : pq[a], x_out = in ? pq[a] : pp[a];
                vertices[(int64_t)v * 3 + a] = x_in + t * (x_out - x_in);
            }
        }
        if (normals) {
            float gq[3], nrm[3];
            iso_gradient(g, f, q, qi, qj, qk, h, gq);
            float big = 0.f;
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float g_in = in ? gp[a] : gq[a], g_out = in ? gq[a] : gp[a];
                nrm[a] = -(g_in + t * (g_out - g_in));
                ok = ok && (fabsf(nrm[a]) <= 3.402823466e38f);
                big = fmaxf(big, fabsf(nrm[a]));
            }
            if (!ok || big == 0.f) {
                nrm[0] = nrm[1] = nrm[2] = 0.f;                          // a gradient that is zero or not finite
            } else {
                nrm[0] /= big; nrm[1] /= big; nrm[2] /= big;             // no overflow / underflow in the squares
                const float len = sqrtf(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
                nrm[0] /= len; nrm[1] /= len; nrm[2] /= len;
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) normals[(int64_t)v * 3 + a] = nrm[a];
        }
        if (vertex_edges) {
            vertex_edges[(int64_t)v * 2] = in ? p : q;
            vertex_edges[(int64_t)v * 2 + 1] = in ? q : p;
        }
        ++v;
    }
}

// pass 4: per lattice point its vertices and, when it is the first corner of a cell, the cell's faces
__global__ void __launch_bounds__(kIsoBlock)
k_iso_emit(IsoGrid g, Lattice box, const float* __restrict__ f, float thr, const unsigned char* __restrict__ mask,
           const unsigned* __restrict__ vbase, const unsigned* __restrict__ block_f, float* __restrict__ vertices,
           float* __restrict__ normals, int* __restrict__ faces, long long* __restrict__ vertex_edges) {
    __shared__ unsigned s_wave[2 * kIsoBlock / 64];
    const int p0 = (blockIdx.x * kIsoBlock + threadIdx.x) * kIsoPer;
    unsigned corners[kIsoPer] = {0, 0, 0, 0}, cnt[kIsoPer] = {0, 0, 0, 0}, nf = 0, unused = 0;
    if (p0 < g.n) {
        const int row = p0 / g.nx;
        int i = p0 - row * g.nx, k = row / g.ny, j = row - k * g.ny;
        for (int r = 0; r < kIsoPer && p0 + r < g.n; ++r) {
            const int p = p0 + r;
            const unsigned m = mask[p];
            if (i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz) {
                corners[r] = iso_cell_corners(m);
                cnt[r] = iso_cell_faces(corners[r]);
                nf += cnt[r];
            }
            if ((m & 0x7fu) && (vertices || normals || vertex_edges))
                iso_emit_vertices(g, box, f, thr, p, i, j, k, m, vbase[p], vertices, normals, vertex_edges);
            if (++i == g.nx) { i = 0; if (++j == g.ny) { j = 0; ++k; } }
        }
    }
    if (!faces) return;                                                  // uniform: a kernel argument
    unsigned tf, tu;
    const unsigned mine = nf;
    iso_block_scan2<kIsoBlock / 64>(nf, unused, s_wave, tf, tu);
    if (mine == 0) return;
    int64_t w = ((int64_t)block_f[blockIdx.x] + nf) * 3;
    for (int r = 0; r < kIsoPer; ++r) {
        if (cnt[r] == 0) continue;
        const int p = p0 + r;
        for (int t = 0; t < 6; ++t) {
            const unsigned c = iso_tet_case(corners[r], t);
            const int nt = c_tet.ntri[t][c];
            for (int q = 0; q < nt; ++q) {
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    const unsigned ed = c_tet.edge[t][c][q][x];
                    const int owner = p + iso_offset(g, ed & 7);
                    const unsigned slot = ed >> 3;
                    faces[w++] = (int)(vbase[owner] + __popc(mask[owner] & ((1u << slot) - 1u)));
                }
            }
        }
    }
}

int64_t iso_num_blocks(int64_t n) { return (n + kIsoTile - 1) / kIsoTile; }

hipError_t launch_iso_count(const int dims[3], const float* f, float thr, unsigned char* mask, unsigned* vbase, unsigned* block_v,
                            unsigned* block_f, unsigned* totals, hipStream_t st) {
    IsoGrid g;
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2];
    g.n = dims[0] * dims[1] * dims[2];
    const unsigned nb = (unsigned)iso_num_blocks(g.n);
    hipLaunchKernelGGL(k_iso_classify, dim3(nb), dim3(kIsoBlock), 0, st, g, f, thr, mask, block_v, block_f);
    hipLaunchKernelGGL(k_iso_scan_blocks, dim3(1), dim3(kIsoScanBlock), 0, st, (int)nb, block_v, block_f, totals);
    hipLaunchKernelGGL(k_iso_bases, dim3(nb), dim3(kIsoBlock), 0, st, g, mask, block_v, vbase);
    return hipGetLastError();
}

hipError_t launch_iso_emit(const int dims[3], const float lo[3], const float hi[3], const float* f, float thr, const unsigned char* mask,
                           const unsigned* vbase, const unsigned* block_f, float* vertices, float* normals, int* faces,
                           long long* vertex_edges, hipStream_t st) {
    IsoGrid g;
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2];
    g.n = dims[0] * dims[1] * dims[2];
    Lattice box;
    box.nx = dims[0]; box.ny = dims[1]; box.nz = dims[2];
    for (int a = 0; a < 3; ++a) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    hipLaunchKernelGGL(k_iso_emit, dim3((unsigned)iso_num_blocks(g.n)), dim3(kIsoBlock), 0, st, g, box, f, thr, mask, vbase, block_f,
                       vertices, normals, faces, vertex_edges);
    return hipGetLastError();
}

}  // namespace mip
