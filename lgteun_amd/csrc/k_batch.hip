// Device-resident dataset (lgteun_amd/resident.py): the one-time PAN pyramid of the whole set and the per-batch gather.
//
//   k_pyr_down2<T>       input_pan_l of every stored PAN plane: two levels of cv2.pyrDown (5 x 5 binomial, BORDER_REFLECT_101, even rows and
//                        columns), dataset.pyr_down(pyr_down(.)).  Integer planes in integer arithmetic -- level 1 times 2^8 is below 2^24, level 2
//                        times 2^16 below 2^32 -- so every sum is exact and the one rounding is the conversion to fp32, like the host's
//                        float64 -> float32; float planes in fp64.
//   k_batch_assemble<T>  one launch per batch: gathers B stored items by a device index list into fresh fp32 NCHW tensors, with the batch's
//                        up-down / left-right flip, 0 - 2 correctly rounded fp32 divisions (dataset normalisation) and an optional fp32 multiply.
//                        A streaming kernel: one 16-byte load per lane (16 uint8 / 8 uint16 / 4 float), float4 stores; a row whose width is not
//                        a multiple of the vector ends in a scalar chunk, and a chunk whose addresses are not 16-byte aligned (rows of such
//                        widths alternate) goes the scalar way too.
//   k_window_assemble<T> the same batch cut out of ONE scene (lgteun_amd/wald.py): item b is the window at origin b of a device list, read
//                        through an origin and the scene's row pitch with ba_chunk -- a window's rows are 16-byte aligned only for some
//                        origins and scene widths, every other chunk goes the scalar way.
//   k_window_pyr<T>      input_pan_l of those windows: pyr_tile, the arithmetic of k_pyr_down2, reflecting at the WINDOW's border, written
//                        flipped and scaled like k_batch_assemble writes the stored pan_l.
#include "abi.h"
#include "common.h"
#include "sample_io.h"

// ------------------------------------------------------------------------------------------------
// pyramid
// ------------------------------------------------------------------------------------------------
#define PYR_T 8                       // level-2 outputs per tile edge
#define PYR_L1 (2 * PYR_T + 3)        // level-1 values per tile edge
#define PYR_NT 256

template <typename T> struct PyrAcc { typedef uint32_t type; };
template <> struct PyrAcc<float> { typedef double type; };

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// One PYR_T x PYR_T tile of level 2 of the H x W plane at p (rows `pitch` samples apart): true for the lanes that hold an output, (oy, ox)
// and its fp32 value v.  Called by every lane of the block (it synchronises).
template <typename T>
__device__ __forceinline__ bool pyr_tile(const T* __restrict__ p, size_t pitch, int H, int W, int oy0, int ox0,
                                         typename PyrAcc<T>::type (&l1)[PYR_L1][PYR_L1 + 1], int& oy, int& ox, float& v) {
    typedef typename PyrAcc<T>::type A;
    constexpr bool INT = !__is_same(T, float);
    const int h1 = H >> 1, w1 = W >> 1, h2 = H >> 2, w2 = W >> 2;
    const A kw[5] = {(A)1, (A)4, (A)6, (A)4, (A)1};
    // level 1 at the (reflected) positions the tile's level-2 taps touch
    for (int t = threadIdx.x; t < PYR_L1 * PYR_L1; t += PYR_NT) {
        const int ry = t / PYR_L1, rx = t - ry * PYR_L1;
        const int py = reflect101(2 * oy0 - 2 + ry, h1), px = reflect101(2 * ox0 - 2 + rx, w1);
        A acc = 0;
        if ((unsigned)py < (unsigned)h1 && (unsigned)px < (unsigned)w1) {   // positions past a partial tile's own taps reflect out of the plane: never read below
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                const T* __restrict__ row = p + (size_t)reflect101(2 * py + a - 2, H) * pitch;
                A r = 0;
#pragma unroll
                for (int b = 0; b < 5; ++b) r += kw[b] * (A)row[reflect101(2 * px + b - 2, W)];
                acc += kw[a] * (INT ? r : r * (A)0.0625);
            }
            if (!INT) acc = acc * (A)0.0625;
        }
        l1[ry][rx] = acc;
    }
    __syncthreads();
    if (threadIdx.x >= PYR_T * PYR_T) return false;
    const int ly = threadIdx.x / PYR_T, lx = threadIdx.x % PYR_T;
    oy = oy0 + ly; ox = ox0 + lx;
    if (oy >= h2 || ox >= w2) return false;
    A acc = 0;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        A r = 0;
#pragma unroll
        for (int b = 0; b < 5; ++b) r += kw[b] * l1[2 * ly + a][2 * lx + b];
        acc += kw[a] * (INT ? r : r * (A)0.0625);
    }
    if (INT) v = (float)acc * (1.0f / 65536.0f);          // round-to-nearest-even conversion, then an exact power of two
    else v = (float)(acc * (A)0.0625);
    return true;
}

template <typename T>
__global__ __launch_bounds__(PYR_NT) void k_pyr_down2(const T* __restrict__ in, float* __restrict__ out, int H, int W, int tiles_x, int tiles) {
    __shared__ typename PyrAcc<T>::type l1[PYR_L1][PYR_L1 + 1];
    const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    int oy, ox;
    float v;
    if (pyr_tile<T>(in + (size_t)plane * H * W, (size_t)W, H, W, ty * PYR_T, tx * PYR_T, l1, oy, ox, v))
        out[(size_t)plane * (H >> 2) * (W >> 2) + (size_t)oy * (W >> 2) + ox] = v;
}

static const char* pyr_check(const void* pan, const float* pan_l, int64_t planes, int H, int W, int dtype) {
    if (!pan || !pan_l) return "null pointer";
    if (dtype < LG_DT_U8 || dtype > LG_DT_F32) return "unknown sample type (LG_DT_U8 / LG_DT_U16 / LG_DT_F32)";
    if (H < 8 || W < 8 || (H & 3) || (W & 3) || H > 32768 || W > 32768) return "H and W must be multiples of 4 in 8 .. 32768";
    const int64_t tiles = (int64_t)((H / 4 + PYR_T - 1) / PYR_T) * ((W / 4 + PYR_T - 1) / PYR_T);
    if (planes <= 0 || planes * tiles > 0x7fffffffll) return "planes must be positive and planes x tiles below 2^31";
    return nullptr;
}

extern "C" int lg_pyr_down2(const void* pan, float* pan_l, int64_t planes, int32_t H, int32_t W, int32_t dtype, void* stream) {
    if (const char* why = pyr_check(pan, pan_l, planes, H, W, dtype)) { lg_set_error("pyr_down2: %s", why); return -1; }
    const int tiles_x = (W / 4 + PYR_T - 1) / PYR_T, tiles = tiles_x * ((H / 4 + PYR_T - 1) / PYR_T);
    const unsigned grid = (unsigned)(planes * tiles);
    const hipStream_t s = (hipStream_t)stream;
    if (dtype == LG_DT_U8) k_pyr_down2<uint8_t><<<grid, PYR_NT, 0, s>>>((const uint8_t*)pan, pan_l, H, W, tiles_x, tiles);
    else if (dtype == LG_DT_U16) k_pyr_down2<uint16_t><<<grid, PYR_NT, 0, s>>>((const uint16_t*)pan, pan_l, H, W, tiles_x, tiles);
    else k_pyr_down2<float><<<grid, PYR_NT, 0, s>>>((const float*)pan, pan_l, H, W, tiles_x, tiles);
    LG_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// batch assembly
// ------------------------------------------------------------------------------------------------
#define BA_NT 256
#define BA_FLIP_UD 1u
#define BA_FLIP_LR 2u

struct BaScale {
    float divisor, post_scale;
    int n_div, has_scale;
};

struct BatchArgs {
    const void *pan, *lr, *mul;       // store: [N,1,H,W], [N,C,h,w], [N,C,H,W] or null
    const float* pan_l;               // store: [N,1,h,w]
    float *o_pan, *o_lr, *o_mul, *o_pan_l;
    const int32_t* idx;               // B store indices of this batch
    const uint32_t* flips;            // the batch's flip word (bit 0 up-down, bit 1 left-right) or null
    int N, C, H, W, h, w;
    BaScale sc;
};

// chunk q of a [planes, rows, width] block of one item: VEC consecutive output elements of one row.  The source planes lie `splane`
// samples apart and their rows `spitch` (a stored item: rows * width and width; a window of a scene: the scene's)
template <typename T>
__device__ __forceinline__ void ba_chunk(const T* __restrict__ src, size_t splane, size_t spitch, float* __restrict__ dst, int rows, int width,
                                         int cpr, int q, uint32_t flips, const BaScale& a) {
    constexpr int V = Vec16<T>::N;
    const int row = q / cpr, c = q - row * cpr;
    const int plane = row / rows, y = row - plane * rows;
    const int ys = (flips & BA_FLIP_UD) ? rows - 1 - y : y;
    const bool lrf = (flips & BA_FLIP_LR) != 0;
    const T* __restrict__ srow = src + (size_t)plane * splane + (size_t)ys * spitch;
    float* __restrict__ drow = dst + ((size_t)plane * rows + y) * width;
    const int e0 = c * V;
    if (e0 + V <= width) {
        const T* sp = srow + (lrf ? width - e0 - V : e0);      // the mirrored chunk, reversed in registers below
        float* dp = drow + e0;
        if ((((uintptr_t)sp | (uintptr_t)dp) & 15) == 0) {
            const uint4 raw = *reinterpret_cast<const uint4*>(sp);
            float f[V];
            unpack16(raw, f, (const T*)nullptr);
#pragma unroll
            for (int i = 0; i < V; ++i) f[i] = ba_scale(f[i], a.divisor, a.n_div, a.post_scale, a.has_scale);
#pragma unroll
            for (int i = 0; i < V; i += 4) {
                const float4 o = lrf ? make_float4(f[V - 1 - i], f[V - 2 - i], f[V - 3 - i], f[V - 4 - i]) : make_float4(f[i], f[i + 1], f[i + 2], f[i + 3]);
                *reinterpret_cast<float4*>(dp + i) = o;
            }
            return;
        }
    }
    const int e1 = e0 + V < width ? e0 + V : width;
    for (int e = e0; e < e1; ++e)
        drow[e] = ba_scale((float)srow[lrf ? width - 1 - e : e], a.divisor, a.n_div, a.post_scale, a.has_scale);
}

template <typename T>
__global__ __launch_bounds__(BA_NT) void k_batch_assemble(const BatchArgs a, int cprW, int cprw, int cprp, int n_pan, int n_mul, int n_lr, int n_pl) {
    constexpr int V = Vec16<T>::N;
    (void)V;
    const int b = blockIdx.y;
    int q = blockIdx.x * BA_NT + threadIdx.x;
    int n = a.idx[b];
    n = n < 0 ? 0 : (n >= a.N ? a.N - 1 : n);              // an index outside the store never becomes an address
    const uint32_t flips = a.flips ? *a.flips : 0u;
    const size_t HW = (size_t)a.H * a.W, hw = (size_t)a.h * a.w;
    if (q < n_pan) {
        ba_chunk<T>((const T*)a.pan + (size_t)n * HW, HW, a.W, a.o_pan + (size_t)b * HW, a.H, a.W, cprW, q, flips, a.sc);
        return;
    }
    q -= n_pan;
    if (q < n_mul) {
        ba_chunk<T>((const T*)a.mul + (size_t)n * a.C * HW, HW, a.W, a.o_mul + (size_t)b * a.C * HW, a.H, a.W, cprW, q, flips, a.sc);
        return;
    }
    q -= n_mul;
    if (q < n_lr) {
        ba_chunk<T>((const T*)a.lr + (size_t)n * a.C * hw, hw, a.w, a.o_lr + (size_t)b * a.C * hw, a.h, a.w, cprw, q, flips, a.sc);
        return;
    }
    q -= n_lr;
    if (q < n_pl) ba_chunk<float>(a.pan_l + (size_t)n * hw, hw, a.w, a.o_pan_l + (size_t)b * hw, a.h, a.w, cprp, q, flips, a.sc);
}

template <typename T>
static void ba_launch(const BatchArgs& a, int B, hipStream_t s) {
    constexpr int V = Vec16<T>::N;
    const int cprW = (a.W + V - 1) / V, cprw = (a.w + V - 1) / V, cprp = (a.w + 3) / 4;
    const int n_pan = a.H * cprW, n_mul = a.mul ? a.C * a.H * cprW : 0, n_lr = a.C * a.h * cprw, n_pl = a.h * cprp;
    const int total = n_pan + n_mul + n_lr + n_pl;
    k_batch_assemble<T><<<dim3((total + BA_NT - 1) / BA_NT, B), BA_NT, 0, s>>>(a, cprW, cprw, cprp, n_pan, n_mul, n_lr, n_pl);
}

extern "C" int lg_batch_assemble(const void* pan, const void* lr, const void* mul, const float* pan_l, int64_t N, const int32_t* idx, int64_t idx_offset,
                                 const uint32_t* flips, float* o_pan, float* o_lr, float* o_mul, float* o_pan_l, int32_t B, int32_t C, int32_t H, int32_t W,
                                 int32_t h, int32_t w, int32_t dtype, float divisor, int32_t n_div, float post_scale, void* stream) {
    const char* why = nullptr;
    if (!pan || !lr || !pan_l || !idx || !o_pan || !o_lr || !o_pan_l || ((mul == nullptr) != (o_mul == nullptr))) why = "null pointer (mul and its output go together)";
    else if (B <= 0 || B > 65535) why = "B must be in 1 .. 65535";
    else if (C < 1 || C > 16) why = "C must be in 1 .. 16";
    else if (h <= 0 || w <= 0 || h > 8192 || w > 8192 || H != 4 * h || W != 4 * w) why = "H and W must be 4 x the MS size (MS up to 8192)";
    else if (dtype < LG_DT_U8 || dtype > LG_DT_F32) why = "unknown sample type (LG_DT_U8 / LG_DT_U16 / LG_DT_F32)";
    else if (n_div < 0 || n_div > 2) why = "the divide count must be 0, 1 or 2";
    else if (n_div > 0 && !(divisor > 0.0f && divisor < INFINITY)) why = "the divisor must be positive and finite";
    else if (!(post_scale == post_scale) || post_scale == INFINITY || post_scale == -INFINITY) why = "the scale must be finite";
    else if (N <= 0 || N > 0x7fffffffll || idx_offset < 0) why = "N must be in 1 .. 2^31 - 1 and the index offset non-negative";
    else if ((int64_t)(C + 1) * H * ((W + 3) / 4) + (int64_t)(C + 1) * h * w > 0x7fffffffll) why = "item too large";
    else if (((uintptr_t)pan | (uintptr_t)lr | (uintptr_t)mul | (uintptr_t)pan_l | (uintptr_t)o_pan | (uintptr_t)o_lr | (uintptr_t)o_mul | (uintptr_t)o_pan_l) & 15)
        why = "store and output arrays must be 16-byte aligned";
    if (why) { lg_set_error("batch_assemble: %s", why); return -1; }
    BatchArgs a;
    a.pan = pan; a.lr = lr; a.mul = mul; a.pan_l = pan_l;
    a.o_pan = o_pan; a.o_lr = o_lr; a.o_mul = o_mul; a.o_pan_l = o_pan_l;
    a.idx = idx + idx_offset; a.flips = flips;
    a.N = (int)N; a.C = C; a.H = H; a.W = W; a.h = h; a.w = w;
    a.sc.divisor = divisor; a.sc.post_scale = post_scale; a.sc.n_div = n_div; a.sc.has_scale = post_scale != 1.0f;
    const hipStream_t s = (hipStream_t)stream;
    ProfScope prof(LG_K_BATCH, s);
    if (dtype == LG_DT_U8) ba_launch<uint8_t>(a, B, s);
    else if (dtype == LG_DT_U16) ba_launch<uint16_t>(a, B, s);
    else ba_launch<float>(a, B, s);
    LG_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// window batches out of one scene
// ------------------------------------------------------------------------------------------------
struct WindowArgs {
    const void *pan, *lr, *mul;       // scene: [1,Hs,Ws], [C,Hs/4,Ws/4], [C,Hs,Ws] or null
    float *o_pan, *o_lr, *o_mul, *o_pan_l;
    const int32_t* org;               // (oy, ox) in PAN pixels of this batch's windows
    const uint32_t* flips;
    int C, Hs, Ws, P, Q;
    BaScale sc;
};

// an origin outside the scene, or off the 4-pixel grid, never becomes an address
__device__ __forceinline__ void wa_origin(const WindowArgs& a, int b, int& oy, int& ox) {
    oy = a.org[2 * b]; ox = a.org[2 * b + 1];
    oy = (oy < 0 ? 0 : (oy > a.Hs - a.P ? a.Hs - a.P : oy)) & ~3;
    ox = (ox < 0 ? 0 : (ox > a.Ws - a.Q ? a.Ws - a.Q : ox)) & ~3;
}

template <typename T>
__global__ __launch_bounds__(BA_NT) void k_window_assemble(const WindowArgs a, int cprW, int cprw, int n_pan, int n_mul, int n_lr) {
    const int b = blockIdx.y;
    int q = blockIdx.x * BA_NT + threadIdx.x;
    int oy, ox;
    wa_origin(a, b, oy, ox);
    const uint32_t flips = a.flips ? *a.flips : 0u;
    const int hs = a.Hs >> 2, ws = a.Ws >> 2, p = a.P >> 2, qq = a.Q >> 2;
    const size_t SP = (size_t)a.Hs * a.Ws, sp = (size_t)hs * ws, PQ = (size_t)a.P * a.Q, pq = (size_t)p * qq;
    if (q < n_pan) {
        ba_chunk<T>((const T*)a.pan + (size_t)oy * a.Ws + ox, SP, a.Ws, a.o_pan + (size_t)b * PQ, a.P, a.Q, cprW, q, flips, a.sc);
        return;
    }
    q -= n_pan;
    if (q < n_mul) {
        ba_chunk<T>((const T*)a.mul + (size_t)oy * a.Ws + ox, SP, a.Ws, a.o_mul + (size_t)b * a.C * PQ, a.P, a.Q, cprW, q, flips, a.sc);
        return;
    }
    q -= n_mul;
    if (q < n_lr) ba_chunk<T>((const T*)a.lr + (size_t)(oy >> 2) * ws + (ox >> 2), sp, ws, a.o_lr + (size_t)b * a.C * pq, p, qq, cprw, q, flips, a.sc);
}

template <typename T>
__global__ __launch_bounds__(PYR_NT) void k_window_pyr(const WindowArgs a, int tiles_x) {
    __shared__ typename PyrAcc<T>::type l1[PYR_L1][PYR_L1 + 1];
    const int b = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    int wy, wx, oy, ox;
    wa_origin(a, b, wy, wx);
    float v;
    if (!pyr_tile<T>((const T*)a.pan + (size_t)wy * a.Ws + wx, (size_t)a.Ws, a.P, a.Q, ty * PYR_T, tx * PYR_T, l1, oy, ox, v)) return;
    const uint32_t flips = a.flips ? *a.flips : 0u;
    const int p = a.P >> 2, qq = a.Q >> 2;
    const int dy = (flips & BA_FLIP_UD) ? p - 1 - oy : oy, dx = (flips & BA_FLIP_LR) ? qq - 1 - ox : ox;      // ba_chunk's flips, from the source's side
    a.o_pan_l[((size_t)b * p + dy) * qq + dx] = ba_scale(v, a.sc.divisor, a.sc.n_div, a.sc.post_scale, a.sc.has_scale);
}

template <typename T>
static void wa_launch(const WindowArgs& a, int B, hipStream_t s) {
    constexpr int V = Vec16<T>::N;
    const int p = a.P / 4, q = a.Q / 4;
    const int cprW = (a.Q + V - 1) / V, cprw = (q + V - 1) / V;
    const int n_pan = a.P * cprW, n_mul = a.mul ? a.C * a.P * cprW : 0, n_lr = a.C * p * cprw;
    k_window_assemble<T><<<dim3((n_pan + n_mul + n_lr + BA_NT - 1) / BA_NT, B), BA_NT, 0, s>>>(a, cprW, cprw, n_pan, n_mul, n_lr);
    const int tiles_x = (q + PYR_T - 1) / PYR_T, tiles_y = (p + PYR_T - 1) / PYR_T;
    k_window_pyr<T><<<dim3(tiles_x * tiles_y, B), PYR_NT, 0, s>>>(a, tiles_x);
}

extern "C" int lg_window_assemble(const void* pan, const void* lr, const void* mul, const int32_t* origins, int64_t n_windows, int64_t first,
                                  const uint32_t* flips, float* o_pan, float* o_lr, float* o_mul, float* o_pan_l, int32_t B, int32_t C, int32_t Hs,
                                  int32_t Ws, int32_t P, int32_t Q, int32_t dtype, float divisor, int32_t n_div, float post_scale, void* stream) {
    const char* why = nullptr;
    if (!pan || !lr || !origins || !o_pan || !o_lr || !o_pan_l || ((mul == nullptr) != (o_mul == nullptr))) why = "null pointer (mul and its output go together)";
    else if (B <= 0 || B > 65535) why = "B must be in 1 .. 65535";
    else if (C < 1 || C > 16) why = "C must be in 1 .. 16";
    else if (Hs < 8 || Ws < 8 || (Hs & 3) || (Ws & 3) || Hs > 65536 || Ws > 65536) why = "scene Hs and Ws must be multiples of 4 in 8 .. 65536";
    else if (P < 8 || Q < 8 || (P & 3) || (Q & 3) || P > 4096 || Q > 4096) why = "window sides must be multiples of 4 in 8 .. 4096";
    else if (P > Hs || Q > Ws) why = "a window side must not exceed the scene side";
    else if (dtype < LG_DT_U8 || dtype > LG_DT_F32) why = "unknown sample type (LG_DT_U8 / LG_DT_U16 / LG_DT_F32)";
    else if (n_div < 0 || n_div > 2) why = "the divide count must be 0, 1 or 2";
    else if (n_div > 0 && !(divisor > 0.0f && divisor < INFINITY)) why = "the divisor must be positive and finite";
    else if (!(post_scale == post_scale) || post_scale == INFINITY || post_scale == -INFINITY) why = "the scale must be finite";
    else if (n_windows <= 0 || n_windows > 0x3fffffffll || first < 0 || first + B > n_windows) why = "windows first .. first + B - 1 must lie inside the origin list (1 .. 2^30 - 1 windows)";
    else if (((uintptr_t)pan | (uintptr_t)lr | (uintptr_t)mul | (uintptr_t)o_pan | (uintptr_t)o_lr | (uintptr_t)o_mul | (uintptr_t)o_pan_l) & 15)
        why = "scene and output arrays must be 16-byte aligned";
    else if (((uintptr_t)origins | (uintptr_t)flips) & 3) why = "the origin list and the flip word must be 4-byte aligned";
    if (why) { lg_set_error("window_assemble: %s", why); return -1; }
    WindowArgs a;
    a.pan = pan; a.lr = lr; a.mul = mul;
    a.o_pan = o_pan; a.o_lr = o_lr; a.o_mul = o_mul; a.o_pan_l = o_pan_l;
    a.org = origins + 2 * first; a.flips = flips;
    a.C = C; a.Hs = Hs; a.Ws = Ws; a.P = P; a.Q = Q;
    a.sc.divisor = divisor; a.sc.post_scale = post_scale; a.sc.n_div = n_div; a.sc.has_scale = post_scale != 1.0f;
    const hipStream_t s = (hipStream_t)stream;
    if (dtype == LG_DT_U8) wa_launch<uint8_t>(a, B, s);
    else if (dtype == LG_DT_U16) wa_launch<uint16_t>(a, B, s);
    else wa_launch<float>(a, B, s);
    LG_CHECK_LAUNCH();
    return 0;
}
