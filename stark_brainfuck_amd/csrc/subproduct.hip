// subproduct.hip -- subproduct tree over an arbitrary set of base-field points: the zerofier, multipoint evaluation and
// interpolation of the reference's fast_zerofier / fast_evaluate / fast_interpolate (ntt.py:82-161), level by level on the device.
//
// The n points are padded to N = 2^L leaves; a padding leaf is the constant polynomial 1, so every node is the exact product of the
// linear factors X - x_i of the real points below it.  Node c of level k covers leaves [c 2^k, (c+1) 2^k) and has degree
// d = clamp(n - c 2^k, 0, 2^k) (node_deg).  Its SLOT is 2^k words: coefficients 0 .. 2^k - 1 of the monic node polynomial; the leading 1 of
// a full node (d = 2^k) sits at index 2^k and is implicit, the 1 of a partial node (d < 2^k) is stored.
//
//   levels 0 .. T      one workgroup per 2^T-leaf subtree, schoolbook products in LDS (leaf_kernel); only level T is kept
//   levels T+1 .. L    batched products through the tile NTT (ntt_launch): forward transforms of size 2^(k+1) of every level-k node
//                      are kept (fz) for the remainder tree and for interpolation's linear-combination tree
//   inverses           rev(node)^-1 mod X^(2^k) for every node of levels T .. L-1 by Newton iteration, batched per level (fi: kept
//                      as size-2^(k+1) transforms)
//   evaluation         polynomial mod root (Newton inverse of the reversed root, only when it has more than n coefficients), then
//                      two products per node down to level T, then Horner at each point on its level-T remainder
//   interpolation      Z'(x_i) by the evaluation above, weights v_i / Z'(x_i) (batch inverse: a zero means two equal points), then
//                      node = C_left Z_right + C_right Z_left bottom up (levels 0 .. T in LDS, above through the kept transforms)
//
// Every transform here is exact: a product of degree < 2^(k+1) in a cyclic convolution of length 2^(k+1), except the product of two
// full children, whose leading 1 wraps onto coefficient 0 and is taken off again (wrap_fix_kernel).
#include "../../include/bfstark.h"

#include "runtime.hpp"

using namespace bfs;

namespace {

constexpr u32 PT_LEAF_LOG = 7;          // bottom subtrees of 128 leaves (levels 0..7 in LDS; Horner over <= 128 coefficients per point)
constexpr u32 PT_THREADS = 256;

__host__ __device__ inline u64 node_deg(u64 n, u32 k, u64 c) {
    const u64 lo = c << k;
    if (lo >= n) return 0;
    const u64 s = 1ull << k;
    return n - lo < s ? n - lo : s;
}

u32 grid_of(u64 work) {
    const u64 g = (work + PT_THREADS - 1) / PT_THREADS;
    return (u32)(g > 4096 ? 4096 : (g ? g : 1));
}

#define PT_LOOP(i, total) for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < (total); i += (u64)gridDim.x * blockDim.x)

// ---- bottom levels: one workgroup per subtree of 2^T leaves.  Node polynomials of level l are kept with all 2^l + 1 coefficients (LDS
// ping-pong).  `w` == null: write the subtree's product into slot form (level T of the tree).  Otherwise column blockIdx.y of the
// weights (N words per column) goes through node = C_left Z_right + C_right Z_left and the level-T combination is written to `out`.
__global__ void __launch_bounds__(PT_THREADS) leaf_kernel(const u64* pts, u64 n, u32 T, const u64* w, u64* out, u64 N) {
    __shared__ u64 z[2][2 << PT_LEAF_LOG];
    __shared__ u64 cb[2][1 << PT_LEAF_LOG];
    const u64 S_T = 1ull << T;
    const u64 base = (u64)blockIdx.x * S_T;
    const u64 col = blockIdx.y;
    const bool interp = w != nullptr;
    for (u32 j = threadIdx.x; j < S_T; j += blockDim.x) {
        const u64 g = base + j;
        z[0][2 * j] = g < n ? gl_neg(pts[g]) : 1;
        z[0][2 * j + 1] = g < n ? 1 : 0;
        if (interp) cb[0][j] = g < n ? w[col * N + g] : 0;
    }
    __syncthreads();
    u32 cur = 0;
    for (u32 l = 0; l < T; ++l) {
        const u64 S = 1ull << l, parents = S_T >> (l + 1);
        const u64* zi = z[cur];
        u64* zo = z[cur ^ 1];
        if (interp) {
            const u64* ci = cb[cur];
            u64* co = cb[cur ^ 1];
            for (u64 idx = threadIdx.x; idx < parents * 2 * S; idx += blockDim.x) {
                const u64 p = idx / (2 * S), c = idx % (2 * S);
                const u64* zl = zi + (2 * p) * (S + 1);
                const u64* zr = zl + (S + 1);
                const u64* cl = ci + (2 * p) * S;
                const u64* cr = cl + S;
                u64 acc = 0;
                const u64 a0 = c > S ? c - S : 0, a1 = c < S - 1 ? c : S - 1;
                for (u64 a = a0; a <= a1; ++a) acc = gl_add(acc, gl_add(gl_mul(cl[a], zr[c - a]), gl_mul(cr[a], zl[c - a])));
                co[idx] = acc;
            }
        }
        for (u64 idx = threadIdx.x; idx < parents * (2 * S + 1); idx += blockDim.x) {
            const u64 p = idx / (2 * S + 1), c = idx % (2 * S + 1);
            const u64* zl = zi + (2 * p) * (S + 1);
            const u64* zr = zl + (S + 1);
            u64 acc = 0;
            const u64 a0 = c > S ? c - S : 0, a1 = c < S ? c : S;
            for (u64 a = a0; a <= a1; ++a) acc = gl_add(acc, gl_mul(zl[a], zr[c - a]));
            zo[idx] = acc;
        }
        __syncthreads();
        cur ^= 1;
    }
    for (u32 c = threadIdx.x; c < S_T; c += blockDim.x) {
        if (interp) out[col * N + base + c] = cb[cur][c];
        else out[base + c] = z[cur][c];       // coefficient S_T (the leading 1 of a full subtree) is implicit in slot form
    }
}

// F[c][i] += X^(2^k) transformed, for every full node c of level k: omega_{2^(k+1)}^(i 2^k) = (-1)^i
__global__ void add_lead_kernel(u64* F, u64 n, u32 k, u64 nodes) {
    const u64 S2 = 2ull << k;
    PT_LOOP(idx, nodes * S2) {
        const u64 c = idx / S2, i = idx % S2;
        if (node_deg(n, k, c) == (1ull << k)) F[idx] = (i & 1) ? gl_sub(F[idx], 1) : gl_add(F[idx], 1);
    }
}

// H[p] = F[2p] * F[2p+1] (vectors of len words)
__global__ void mul_pairs_kernel(const u64* F, u64* H, u64 len, u64 parents) {
    PT_LOOP(idx, parents * len) {
        const u64 p = idx / len, i = idx % len;
        H[idx] = gl_mul(F[(2 * p) * len + i], F[(2 * p + 1) * len + i]);
    }
}

// the product of two full children has degree 2^(k+1): its leading 1 wrapped onto coefficient 0 of the cyclic product
__global__ void wrap_fix_kernel(u64* z, u64 n, u32 k, u64 nodes) {
    PT_LOOP(c, nodes) if (node_deg(n, k, c) == (1ull << k)) z[c << k] = gl_sub(z[c << k], 1);
}

// f[c][i] = coefficient i of X^d node_c(1/X) (the reversed node, constant term 1), i < flen
__global__ void rev_node_kernel(const u64* z, u64 n, u32 k, u64 nodes, u64 first, u64* f, u64 flen) {
    const u64 S = 1ull << k;
    PT_LOOP(idx, nodes * flen) {
        const u64 c = first + idx / flen, i = idx % flen;
        const u64 d = node_deg(n, k, c);
        f[idx] = i > d ? 0 : (d - i == S ? 1 : z[c * S + d - i]);
    }
}

// dst[r][i] = i < slen ? src[r][i] : 0, i < dlen
__global__ void copy_rows_kernel(const u64* src, u64 ss, u64 slen, u64* dst, u64 ds, u64 dlen, u64 rows) {
    PT_LOOP(idx, rows * dlen) {
        const u64 r = idx / dlen, i = idx % dlen;
        dst[r * ds + i] = i < slen ? src[r * ss + i] : 0;
    }
}

// dst[r][i] = i < cnt ? src[r][top - i] : 0, i < dlen      (a reversal: coefficient i of X^top a(1/X), cut at X^cnt)
__global__ void reverse_rows_kernel(const u64* src, u64 ss, u64 top, u64 cnt, u64* dst, u64 ds, u64 dlen, u64 rows) {
    PT_LOOP(idx, rows * dlen) {
        const u64 r = idx / dlen, i = idx % dlen;
        dst[r * ds + i] = i < cnt && i <= top ? src[r * ss + top - i] : 0;
    }
}

// x[v][i] *= y[v % ny][i]
__global__ void mul_bcast_kernel(u64* x, const u64* y, u64 len, u64 count, u64 ny) {
    PT_LOOP(idx, count * len) {
        const u64 v = idx / len, i = idx % len;
        x[idx] = gl_mul(x[idx], y[(v % ny) * len + i]);
    }
}

// Newton step on transforms: g <- g (2 - f g)
__global__ void newton_kernel(const u64* f, u64* g, u64 total) {
    PT_LOOP(i, total) g[i] = gl_mul(g[i], gl_sub(2, gl_mul(f[i], g[i])));
}

__global__ void set_one_kernel(u64* g, u64 stride, u64 rows) {
    PT_LOOP(r, rows) g[r * stride] = 1;
}

// remainder tree, step 1: W[b][c] = the first min(S, d_parent) coefficients of X^(d_parent - 1) r_parent(1/X), zero padded to 2S
__global__ void rem_prep_kernel(const u64* R, u64 N, u64 n, u32 k, u64 nodes, u64 batch, u64* W) {
    const u64 S = 1ull << k, S2 = 2 * S;
    PT_LOOP(idx, batch * nodes * S2) {
        const u64 v = idx / S2, i = idx % S2, b = v / nodes, c = v % nodes, p = c >> 1;
        const u64 dp = node_deg(n, k + 1, p);
        W[idx] = i < S && i < dp ? R[b * N + p * S2 + dp - 1 - i] : 0;
    }
}

// step 2: quotient q = coefficients ql-1 .. 0 of the product, reversed; ql = d_parent - d_child <= S
__global__ void rem_quot_kernel(const u64* Bv, u64 n, u32 k, u64 nodes, u64 batch, u64* Q) {
    const u64 S = 1ull << k, S2 = 2 * S;
    PT_LOOP(idx, batch * nodes * S2) {
        const u64 v = idx / S2, j = idx % S2, c = v % nodes;
        const u64 d = node_deg(n, k, c), dp = node_deg(n, k + 1, c >> 1);
        const u64 ql = d ? dp - d : 0;
        Q[idx] = j < ql ? Bv[v * S2 + ql - 1 - j] : 0;
    }
}

// step 3: r_child = (r_parent - q node) mod X^d
__global__ void rem_out_kernel(const u64* R, const u64* QM, u64 N, u64 n, u32 k, u64 nodes, u64 batch, u64* Rk) {
    const u64 S = 1ull << k, S2 = 2 * S;
    PT_LOOP(idx, batch * N) {
        const u64 b = idx / N, c = (idx % N) >> k, i = idx & (S - 1);
        const u64 d = node_deg(n, k, c);
        Rk[idx] = i < d ? gl_sub(R[b * N + (c >> 1) * S2 + i], QM[(b * nodes + c) * S2 + i]) : 0;
    }
}

// out[b][i] = r_{i >> T}(x_i) for the level-T remainders
__global__ void horner_kernel(const u64* R, u64 N, u32 T, const u64* pts, u64 n, u64 batch, u64* out, u64 out_stride) {
    const u64 S_T = 1ull << T;
    PT_LOOP(idx, batch * n) {
        const u64 b = idx / n, i = idx % n;
        const u64* r = R + b * N + ((i >> T) << T);
        const u64 x = pts[i];
        u64 acc = 0;
        for (u64 c = S_T; c-- > 0;) acc = gl_add(gl_mul(acc, x), r[c]);
        out[b * out_stride + i] = acc;
    }
}

// root subtraction for a polynomial with more than n coefficients: R[b][i] = P[b][i] - (q Z)[b][i], i < n; zero up to N
__global__ void sub_rows_kernel(const u64* P, u64 ps, const u64* QZ, u64 qs, u64 n, u64 N, u64 batch, u64* R) {
    PT_LOOP(idx, batch * N) {
        const u64 b = idx / N, i = idx % N;
        R[idx] = i < n ? gl_sub(P[b * ps + i], QZ[b * qs + i]) : 0;
    }
}

// the root with its leading 1 written out: n + 1 coefficients
__global__ void root_full_kernel(const u64* z, u64 n, u64* out, u64 len) {
    PT_LOOP(i, len) out[i] = i < n ? z[i] : (i == n ? 1 : 0);
}

// Z'(X): coefficient i = (i + 1) Z_{i+1}, i < n
__global__ void derivative_kernel(const u64* z, u64 n, u64* out) {
    PT_LOOP(i, n) out[i] = gl_mul(gl_canon(i + 1), i + 1 == n ? 1 : z[i + 1]);
}

// weights W[b][i] = v[b][i] / Z'(x_i) (zinv holds the inverses), zero on padding leaves
__global__ void weights_kernel(const u64* v, u64 vs, const u64* zinv, u64 n, u64 N, u64 batch, u64* W) {
    PT_LOOP(idx, batch * N) {
        const u64 b = idx / N, i = idx % N;
        W[idx] = i < n ? gl_mul(v[b * vs + i], zinv[i]) : 0;
    }
}

// H[b][p] = Fc[b][2p] Fz[2p+1] + Fc[b][2p+1] Fz[2p]       (transforms of size len)
__global__ void comb_kernel(const u64* Fc, const u64* Fz, u64 len, u64 parents, u64 batch, u64* H) {
    PT_LOOP(idx, batch * parents * len) {
        const u64 v = idx / len, i = idx % len, b = v / parents, p = v % parents;
        const u64* fl = Fc + (b * 2 * parents + 2 * p) * len;
        H[idx] = gl_add(gl_mul(fl[i], Fz[(2 * p + 1) * len + i]), gl_mul(fl[len + i], Fz[(2 * p) * len + i]));
    }
}

#define PT_LAUNCH(kern, work, ...)                                                                           \
    do {                                                                                                     \
        hipLaunchKernelGGL(kern, dim3(grid_of(work)), dim3(PT_THREADS), 0, stream, __VA_ARGS__);             \
        BFS_HIP(hipGetLastError());                                                                          \
    } while (0)

int fwd(const u64* in, u64 n_in, u64 in_stride, u64* out, u32 log, u64 batch, hipStream_t stream) {
    if (batch > 0xFFFFFFFFull) { set_error("subproduct tree: transform batch too large"); return BFS_ERR_BAD_ARG; }
    return ntt_launch(in, n_in, in_stride, out, 1ull << log, log, (u32)batch, gl_primitive_root(log), 1, 1, stream);
}

int inv(const u64* in, u64* out, u32 log, u64 batch, hipStream_t stream) {
    if (batch > 0xFFFFFFFFull) { set_error("subproduct tree: transform batch too large"); return BFS_ERR_BAD_ARG; }
    const u64 len = 1ull << log;
    return ntt_launch(in, len, len, out, len, log, (u32)batch, gl_inv(gl_primitive_root(log)), 1, gl_inv(len), stream);
}

u32 log2_ceil(u64 x) {
    u32 l = 0;
    while ((1ull << l) < x) ++l;
    return l;
}

// temporaries from the library pool, handed back stream-ordered when the call returns
struct Tmp {
    hipStream_t stream;
    void* blocks[16] = {};
    int count = 0;
    explicit Tmp(hipStream_t s) : stream(s) {}
    int get(u64 words, u64** out) {
        void* p = nullptr;
        BFS_TRY(device_alloc((words ? words : 1) * sizeof(u64), stream, &p));
        blocks[count++] = p;
        *out = (u64*)p;
        return BFS_OK;
    }
    ~Tmp() { for (int i = 0; i < count; ++i) (void)device_release(blocks[i], stream); }
    Tmp(const Tmp&) = delete;
    Tmp& operator=(const Tmp&) = delete;
};

// g[r] = f[r]^-1 mod X^prec for `rows` power series with f[r][0] = 1 (f: rows x fstride words, the first min(fstride, prec) read;
// g: rows x prec words).  g <- g (2 - f g) mod X^(2m), m = 1, 2, .., prec / 2, in transforms of size 4m.
int newton_inverse(const u64* f, u64 fstride, u64* g, u64 prec, u64 rows, hipStream_t stream) {
    Tmp tmp(stream);
    u64 *A = nullptr, *G = nullptr;
    BFS_TRY(tmp.get(rows * 2 * prec, &A));
    BFS_TRY(tmp.get(rows * 2 * prec, &G));
    PT_LAUNCH(copy_rows_kernel, rows * prec, g, prec, (u64)0, g, prec, prec, rows);
    PT_LAUNCH(set_one_kernel, rows, g, prec, rows);
    for (u64 m = 1; m < prec; m *= 2) {
        const u32 lg = log2_ceil(4 * m);
        const u64 fl = 2 * m < fstride ? 2 * m : fstride;
        BFS_TRY(fwd(f, fl, fstride, A, lg, rows, stream));
        BFS_TRY(fwd(g, m, prec, G, lg, rows, stream));
        PT_LAUNCH(newton_kernel, rows * 4 * m, A, G, rows * 4 * m);
        BFS_TRY(inv(G, A, lg, rows, stream));
        PT_LAUNCH(copy_rows_kernel, rows * 2 * m, A, 4 * m, 2 * m, g, prec, 2 * m, rows);
    }
    return BFS_OK;
}

}  // namespace

struct bfs_ptree {
    u64 n = 0, N = 0;
    u32 L = 0, T = 0;
    hipStream_t stream = nullptr;   // the stream the blocks came from (bfs_ptree_free hands them back on the caller's)
    u64* pts = nullptr;             // N words, the points (padding: 0, never read)
    u64* z[33] = {};                // level k = T .. L: N words of slots
    u64* fz[33] = {};               // level k = T .. L-1: 2N words, size-2^(k+1) transforms of the node polynomials
    u64* fi[33] = {};               // level k = T .. L-1: 2N words, size-2^(k+1) transforms of rev(node)^-1 mod X^(2^k)
    void* blocks[100] = {};
    int nblocks = 0;
    int alloc(u64 words, u64** out) {
        void* p = nullptr;
        BFS_TRY(device_alloc(words * sizeof(u64), stream, &p));
        blocks[nblocks++] = p;
        *out = (u64*)p;
        return BFS_OK;
    }
};

namespace {

int ptree_release(bfs_ptree* t, hipStream_t stream) {
    int rc = BFS_OK;
    for (int i = 0; i < t->nblocks; ++i) {
        const int r = device_release(t->blocks[i], stream);
        if (r && !rc) rc = r;
    }
    delete t;
    return rc;
}

int ptree_build(bfs_ptree* t, const u64* d_points, hipStream_t stream) {
    const u64 n = t->n, N = t->N;
    const u32 L = t->L, T = t->T;
    BFS_TRY(t->alloc(N, &t->pts));
    PT_LAUNCH(copy_rows_kernel, N, d_points, (u64)0, n, t->pts, (u64)0, N, (u64)1);
    for (u32 k = T; k <= L; ++k) BFS_TRY(t->alloc(N, &t->z[k]));
    for (u32 k = T; k < L; ++k) {
        BFS_TRY(t->alloc(2 * N, &t->fz[k]));
        BFS_TRY(t->alloc(2 * N, &t->fi[k]));
    }
    hipLaunchKernelGGL(leaf_kernel, dim3((u32)(N >> T), 1), dim3(PT_THREADS), 0, stream, t->pts, n, T, (const u64*)nullptr, t->z[T], N);
    BFS_HIP(hipGetLastError());
    Tmp tmp(stream);
    u64 *H = nullptr, *f = nullptr, *g = nullptr;
    BFS_TRY(tmp.get(N, &H));
    BFS_TRY(tmp.get(N, &f));
    BFS_TRY(tmp.get(N, &g));
    for (u32 k = T; k < L; ++k) {
        const u64 S = 1ull << k, nodes = N >> k;
        // products: level k -> k + 1
        BFS_TRY(fwd(t->z[k], S, S, t->fz[k], k + 1, nodes, stream));
        PT_LAUNCH(add_lead_kernel, 2 * N, t->fz[k], n, k, nodes);
        PT_LAUNCH(mul_pairs_kernel, N, t->fz[k], H, 2 * S, nodes / 2);
        BFS_TRY(inv(H, t->z[k + 1], k + 1, nodes / 2, stream));
        PT_LAUNCH(wrap_fix_kernel, nodes / 2, t->z[k + 1], n, k + 1, nodes / 2);
        // inverses of the reversed level-k nodes mod X^S
        PT_LAUNCH(rev_node_kernel, N, t->z[k], n, k, nodes, (u64)0, f, S);
        BFS_TRY(newton_inverse(f, S, g, S, nodes, stream));
        BFS_TRY(fwd(g, S, S, t->fi[k], k + 1, nodes, stream));
    }
    return BFS_OK;
}

// out[b] (n values, out_stride apart) = P_b(x_i) for `batch` polynomials of m coefficients (in_stride apart)
int ptree_evaluate(const bfs_ptree* t, const u64* P, u64 m, u64 in_stride, u64 batch, u64* out, u64 out_stride, hipStream_t stream) {
    const u64 n = t->n, N = t->N;
    const u32 L = t->L, T = t->T;
    Tmp tmp(stream);
    u64 *R0 = nullptr, *R1 = nullptr;
    BFS_TRY(tmp.get(batch * N, &R0));
    BFS_TRY(tmp.get(batch * N, &R1));
    if (m <= n) {
        PT_LAUNCH(copy_rows_kernel, batch * N, P, in_stride, m, R0, N, N, batch);
    } else {
        // P mod Z: q = rev(rev(P) rev(Z)^-1 mod X^(m-n)), remainder = P - q Z mod X^n (univariate.py divide, as ntt.py:111-114 uses it)
        const u64 ql = m - n, prec = 1ull << log2_ceil(ql);
        u64 *f = nullptr, *g = nullptr, *A = nullptr, *Gt = nullptr;
        BFS_TRY(tmp.get(prec, &f));
        BFS_TRY(tmp.get(prec, &g));
        PT_LAUNCH(rev_node_kernel, prec, t->z[L], n, L, (u64)1, (u64)0, f, prec);
        BFS_TRY(newton_inverse(f, prec, g, prec, 1, stream));
        const u32 l1 = log2_ceil(2 * prec);
        const u32 l2 = log2_ceil(m);
        const u64 w = 1ull << (l1 > l2 ? l1 : l2);
        BFS_TRY(tmp.get(batch * w, &A));
        BFS_TRY(tmp.get(w, &Gt));
        const u64 s1 = 1ull << l1;
        PT_LAUNCH(reverse_rows_kernel, batch * s1, P, in_stride, m - 1, ql, A, s1, s1, batch);
        BFS_TRY(fwd(A, s1, s1, A, l1, batch, stream));
        BFS_TRY(fwd(g, prec, prec, Gt, l1, 1, stream));
        PT_LAUNCH(mul_bcast_kernel, batch * s1, A, Gt, s1, batch, (u64)1);
        BFS_TRY(inv(A, A, l1, batch, stream));
        const u64 s2 = 1ull << l2;
        u64* Q = R1;                                    // batch * s2 words needed: s2 <= w, R1 holds batch * N only when s2 <= N
        u64* Qb = nullptr;
        if (s2 > N) { BFS_TRY(tmp.get(batch * s2, &Qb)); Q = Qb; }
        PT_LAUNCH(reverse_rows_kernel, batch * s2, A, s1, ql - 1, ql, Q, s2, s2, batch);
        BFS_TRY(fwd(Q, s2, s2, Q, l2, batch, stream));
        PT_LAUNCH(root_full_kernel, n + 1, t->z[L], n, Gt, n + 1);
        BFS_TRY(fwd(Gt, n + 1, n + 1, Gt, l2, 1, stream));
        PT_LAUNCH(mul_bcast_kernel, batch * s2, Q, Gt, s2, batch, (u64)1);
        BFS_TRY(inv(Q, Q, l2, batch, stream));
        PT_LAUNCH(sub_rows_kernel, batch * N, P, in_stride, Q, s2, n, N, batch, R0);
    }
    if (L > T) {
        u64 *X1 = nullptr, *X2 = nullptr;
        BFS_TRY(tmp.get(batch * 2 * N, &X1));
        BFS_TRY(tmp.get(batch * 2 * N, &X2));
        for (u32 k = L; k-- > T;) {
            const u64 nodes = N >> k, vecs = batch * nodes;
            PT_LAUNCH(rem_prep_kernel, batch * 2 * N, R0, N, n, k, nodes, batch, X1);
            BFS_TRY(fwd(X1, 2ull << k, 2ull << k, X2, k + 1, vecs, stream));
            PT_LAUNCH(mul_bcast_kernel, batch * 2 * N, X2, t->fi[k], 2ull << k, vecs, nodes);
            BFS_TRY(inv(X2, X1, k + 1, vecs, stream));
            PT_LAUNCH(rem_quot_kernel, batch * 2 * N, X1, n, k, nodes, batch, X2);
            BFS_TRY(fwd(X2, 2ull << k, 2ull << k, X1, k + 1, vecs, stream));
            PT_LAUNCH(mul_bcast_kernel, batch * 2 * N, X1, t->fz[k], 2ull << k, vecs, nodes);
            BFS_TRY(inv(X1, X2, k + 1, vecs, stream));
            PT_LAUNCH(rem_out_kernel, batch * N, R0, X2, N, n, k, nodes, batch, R1);
            u64* s = R0; R0 = R1; R1 = s;
        }
    }
    PT_LAUNCH(horner_kernel, batch * n, R0, N, T, t->pts, n, batch, out, out_stride);
    return BFS_OK;
}

int ptree_interpolate(const bfs_ptree* t, const u64* V, u64 in_stride, u64 batch, u64* out, u64 out_stride, hipStream_t stream) {
    const u64 n = t->n, N = t->N;
    const u32 L = t->L, T = t->T;
    Tmp tmp(stream);
    u64 *zp = nullptr, *e = nullptr, *W = nullptr, *C = nullptr;
    BFS_TRY(tmp.get(n, &zp));
    BFS_TRY(tmp.get(n, &e));
    PT_LAUNCH(derivative_kernel, n, t->z[L], n, zp);
    BFS_TRY(ptree_evaluate(t, zp, n, n, 1, e, n, stream));
    const int rc = batch_inverse_launch(e, e, n, stream);     // Z'(x_i) = 0 <=> x_i occurs twice
    if (rc) return rc;
    BFS_TRY(tmp.get(batch * N, &W));
    BFS_TRY(tmp.get(batch * N, &C));
    PT_LAUNCH(weights_kernel, batch * N, V, in_stride, e, n, N, batch, W);
    if (batch > 65535) { set_error("bfs_ptree_interpolate: more than 65535 columns"); return BFS_ERR_BAD_ARG; }
    hipLaunchKernelGGL(leaf_kernel, dim3((u32)(N >> T), (u32)batch), dim3(PT_THREADS), 0, stream, t->pts, n, T, (const u64*)W, C, N);
    BFS_HIP(hipGetLastError());
    if (L > T) {
        u64* X = nullptr;
        BFS_TRY(tmp.get(batch * 2 * N, &X));
        for (u32 k = T; k < L; ++k) {
            const u64 S = 1ull << k, nodes = N >> k;
            BFS_TRY(fwd(C, S, S, X, k + 1, batch * nodes, stream));
            PT_LAUNCH(comb_kernel, batch * N, X, t->fz[k], 2 * S, nodes / 2, batch, W);
            BFS_TRY(inv(W, C, k + 1, batch * nodes / 2, stream));
        }
    }
    PT_LAUNCH(copy_rows_kernel, batch * n, C, N, n, out, out_stride, n, batch);
    return BFS_OK;
}

}  // namespace

extern "C" {

int bfs_ptree_build(const uint64_t* d_points, uint64_t n, void* stream, bfs_ptree** out) {
    if (!out || !d_points || n == 0) { set_error("bfs_ptree_build: need n >= 1 points and an output handle"); return BFS_ERR_BAD_ARG; }
    *out = nullptr;
    const u32 L = log2_ceil(n);
    if (L > 30) { set_error("bfs_ptree_build: %llu points is too many", (unsigned long long)n); return BFS_ERR_BAD_ARG; }
    bfs_ptree* t = new bfs_ptree;
    t->n = n; t->L = L; t->N = 1ull << L; t->T = L < PT_LEAF_LOG ? L : PT_LEAF_LOG; t->stream = (hipStream_t)stream;
    const int rc = ptree_build(t, d_points, (hipStream_t)stream);
    if (rc) { (void)ptree_release(t, (hipStream_t)stream); return rc; }
    *out = t;
    return BFS_OK;
}

uint64_t bfs_ptree_size(const bfs_ptree* tree) { return tree ? tree->n : 0; }

int bfs_ptree_zerofier(const bfs_ptree* tree, uint64_t* d_out, void* stream) {
    if (!tree || !d_out) { set_error("bfs_ptree_zerofier: null argument"); return BFS_ERR_BAD_ARG; }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(root_full_kernel, dim3(grid_of(tree->n + 1)), dim3(PT_THREADS), 0, s, tree->z[tree->L], tree->n, d_out, tree->n + 1);
    BFS_HIP(hipGetLastError());
    return BFS_OK;
}

int bfs_ptree_evaluate(const bfs_ptree* tree, const uint64_t* d_coeffs, uint64_t n_coeffs, uint64_t in_stride, uint32_t batch,
                       uint64_t* d_out, uint64_t out_stride, void* stream) {
    if (!tree || !d_out || (n_coeffs && !d_coeffs)) { set_error("bfs_ptree_evaluate: null argument"); return BFS_ERR_BAD_ARG; }
    if (batch == 0) return BFS_OK;
    if (batch > 1 && (in_stride < n_coeffs || out_stride < tree->n)) { set_error("bfs_ptree_evaluate: columns overlap"); return BFS_ERR_BAD_ARG; }
    return ptree_evaluate(tree, d_coeffs, n_coeffs, in_stride, batch, d_out, out_stride, (hipStream_t)stream);
}

int bfs_ptree_interpolate(const bfs_ptree* tree, const uint64_t* d_values, uint64_t in_stride, uint32_t batch, uint64_t* d_out,
                          uint64_t out_stride, void* stream) {
    if (!tree || !d_out || !d_values) { set_error("bfs_ptree_interpolate: null argument"); return BFS_ERR_BAD_ARG; }
    if (batch == 0) return BFS_OK;
    if (batch > 1 && (in_stride < tree->n || out_stride < tree->n)) { set_error("bfs_ptree_interpolate: columns overlap"); return BFS_ERR_BAD_ARG; }
    return ptree_interpolate(tree, d_values, in_stride, batch, d_out, out_stride, (hipStream_t)stream);
}

int bfs_ptree_free(bfs_ptree* tree, void* stream) {
    if (!tree) return BFS_OK;
    return ptree_release(tree, (hipStream_t)stream);
}

}  // extern "C"
