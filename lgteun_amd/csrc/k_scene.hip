// Tiled scene fusion (lgteun_amd/scene.py): the bandwidth kernels around the forward for images larger than one plan.
//
//   k_scene_gather<T>  one launch per tile batch: cuts B tiles out of the device-resident scene (PAN [1,H,W], MS [C,H/4,W/4] in the files'
//                      sample type) at the origins of a device list and writes them as fp32 with ba_scale's arithmetic (sample_io.h, shared
//                      with k_batch_assemble).  A lane owns one 16-byte load where source and destination are 16-byte aligned; origins are
//                      multiples of 4 PAN pixels only, so other chunks go quad by quad: one load of 4 samples where the source is aligned
//                      to that, 4 scalar loads otherwise (MS rows), and always one float4 store (destination rows are multiples of 4 floats).
//   k_scene_blend      adds one batch of tile outputs into the fp32 scene with the separable window of scene.py.  No atomics and no
//                      memset: a lane owns 4 consecutive pixels of one tile and goes on only if its tile is the lowest-index tile OF THE
//                      BATCH that covers them; it then walks the batch's covering tiles (at most 3 per axis) in ascending index.  The
//                      cover set is a function of the coordinates (tile boundaries are multiples of 4: the 4 pixels share it), so the
//                      lane knows whether an earlier launch left a partial sum in the scene (it continues that fma chain) and whether a
//                      later launch will add to it (it leaves the sum) or this one holds the last cover (it divides by the weight sum).
//   k_scene_to_u16     clip(rint(x * scale), 0, 65535): the fused scene as digital numbers, 2 bytes per sample.
#include "abi.h"
#include "common.h"
#include "sample_io.h"

#define SC_NT 256

// ------------------------------------------------------------------------------------------------
// gather
// ------------------------------------------------------------------------------------------------
struct SceneGatherArgs {
    const void *pan, *ms;             // scene: [1,H,W], [C,H/4,W/4]
    const int32_t* org;               // (oy, ox) in PAN pixels of this batch's tiles
    float *o_pan, *o_ms;              // [B,1,th,tw], [B,C,th/4,tw/4]
    int C, H, W, th, tw;
    float divisor, post_scale;
    int n_div, has_scale;
};

// 4 consecutive samples as floats: one load where the address allows it
__device__ __forceinline__ void sg_load4(const uint8_t* p, float (&f)[4]) {
    if (((uintptr_t)p & 3) == 0) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = (float)((w >> (8 * i)) & 0xffu);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = (float)p[i];
    }
}
__device__ __forceinline__ void sg_load4(const uint16_t* p, float (&f)[4]) {
    if (((uintptr_t)p & 7) == 0) {
        const uint2 w = *reinterpret_cast<const uint2*>(p);
        f[0] = (float)(w.x & 0xffffu); f[1] = (float)(w.x >> 16); f[2] = (float)(w.y & 0xffffu); f[3] = (float)(w.y >> 16);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = (float)p[i];
    }
}
__device__ __forceinline__ void sg_load4(const float* p, float (&f)[4]) {
    if (((uintptr_t)p & 15) == 0) {
        const float4 w = *reinterpret_cast<const float4*>(p);
        f[0] = w.x; f[1] = w.y; f[2] = w.z; f[3] = w.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = p[i];
    }
}

// chunk q of one tile's [planes, rows, width] block: up to VEC consecutive output elements of one row; the source is the window at
// (sy, sx) of a [planes, srows, swidth] array.  width is a multiple of 4 and dst is 16-byte aligned: every quad of a row is a float4.
template <typename T>
__device__ __forceinline__ void sg_chunk(const T* __restrict__ src, float* __restrict__ dst, int rows, int width, int srows, int swidth,
                                         int sy, int sx, int cpr, int q, const SceneGatherArgs& a) {
    constexpr int V = Vec16<T>::N;
    const int row = q / cpr, c = q - row * cpr;
    const int plane = row / rows, y = row - plane * rows;
    const T* __restrict__ srow = src + ((size_t)plane * srows + sy + y) * swidth + sx;
    float* __restrict__ drow = dst + ((size_t)plane * rows + y) * width;
    const int e0 = c * V;
    if (e0 + V <= width && (((uintptr_t)(srow + e0) | (uintptr_t)(drow + e0)) & 15) == 0) {
        const uint4 raw = *reinterpret_cast<const uint4*>(srow + e0);
        float f[V];
        unpack16(raw, f, (const T*)nullptr);
#pragma unroll
        for (int i = 0; i < V; ++i) f[i] = ba_scale(f[i], a.divisor, a.n_div, a.post_scale, a.has_scale);
#pragma unroll
        for (int i = 0; i < V; i += 4) *reinterpret_cast<float4*>(drow + e0 + i) = make_float4(f[i], f[i + 1], f[i + 2], f[i + 3]);
        return;
    }
    const int e1 = e0 + V < width ? e0 + V : width;
    for (int e = e0; e < e1; e += 4) {
        float f[4];
        sg_load4(srow + e, f);
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = ba_scale(f[i], a.divisor, a.n_div, a.post_scale, a.has_scale);
        *reinterpret_cast<float4*>(drow + e) = make_float4(f[0], f[1], f[2], f[3]);
    }
}

template <typename T>
__global__ __launch_bounds__(SC_NT) void k_scene_gather(const SceneGatherArgs a, int cprW, int cprw, int n_pan, int n_ms) {
    const int b = blockIdx.y;
    int q = blockIdx.x * SC_NT + threadIdx.x;
    // an origin outside the scene, or off the 4-pixel grid, never becomes an address
    int oy = a.org[2 * b], ox = a.org[2 * b + 1];
    oy = (oy < 0 ? 0 : (oy > a.H - a.th ? a.H - a.th : oy)) & ~3;
    ox = (ox < 0 ? 0 : (ox > a.W - a.tw ? a.W - a.tw : ox)) & ~3;
    const int h = a.H >> 2, w = a.W >> 2, tth = a.th >> 2, ttw = a.tw >> 2;
    if (q < n_pan) {
        sg_chunk<T>((const T*)a.pan, a.o_pan + (size_t)b * a.th * a.tw, a.th, a.tw, a.H, a.W, oy, ox, cprW, q, a);
        return;
    }
    q -= n_pan;
    if (q < n_ms) sg_chunk<T>((const T*)a.ms, a.o_ms + (size_t)b * a.C * tth * ttw, tth, ttw, h, w, oy >> 2, ox >> 2, cprw, q, a);
}

template <typename T>
static void sg_launch(const SceneGatherArgs& a, int B, hipStream_t s) {
    constexpr int V = Vec16<T>::N;
    const int cprW = (a.tw + V - 1) / V, cprw = (a.tw / 4 + V - 1) / V;
    const int n_pan = a.th * cprW, n_ms = a.C * (a.th / 4) * cprw;
    k_scene_gather<T><<<dim3((n_pan + n_ms + SC_NT - 1) / SC_NT, B), SC_NT, 0, s>>>(a, cprW, cprw, n_pan, n_ms);
}

static const char* scene_shape_check(int C, int H, int W, int th, int tw) {
    if (C < 1 || C > 16) return "C must be in 1 .. 16";
    if (H < 16 || W < 16 || (H & 3) || (W & 3) || H > 65536 || W > 65536) return "scene H and W must be multiples of 4 in 16 .. 65536";
    if (th < 16 || tw < 16 || (th & 15) || (tw & 15) || th > 1024 || tw > 1024) return "tile sides must be multiples of 16 in 16 .. 1024";
    if (th > H || tw > W) return "a tile side must not exceed the scene side";
    return nullptr;
}

extern "C" int lg_scene_gather(const void* pan, const void* ms, const int32_t* origins, int64_t n_tiles, int64_t first, float* o_pan, float* o_ms,
                               int32_t B, int32_t C, int32_t H, int32_t W, int32_t th, int32_t tw, int32_t dtype, float divisor, int32_t n_div,
                               float post_scale, void* stream) {
    const char* why = nullptr;
    if (!pan || !ms || !origins || !o_pan || !o_ms) why = "null pointer";
    else if (B <= 0 || B > 65535) why = "B must be in 1 .. 65535";
    else if ((why = scene_shape_check(C, H, W, th, tw)) != nullptr) {}
    else if (dtype < LG_DT_U8 || dtype > LG_DT_F32) why = "unknown sample type (LG_DT_U8 / LG_DT_U16 / LG_DT_F32)";
    else if (n_div < 0 || n_div > 2) why = "the divide count must be 0, 1 or 2";
    else if (n_div > 0 && !(divisor > 0.0f && divisor < INFINITY)) why = "the divisor must be positive and finite";
    else if (!(post_scale == post_scale) || post_scale == INFINITY || post_scale == -INFINITY) why = "the scale must be finite";
    else if (n_tiles <= 0 || n_tiles > 0x3fffffffll || first < 0 || first + B > n_tiles) why = "tiles first .. first + B - 1 must lie inside the origin list (1 .. 2^30 - 1 tiles)";
    else if (((uintptr_t)pan | (uintptr_t)ms | (uintptr_t)o_pan | (uintptr_t)o_ms) & 15) why = "scene and tile arrays must be 16-byte aligned";
    else if ((uintptr_t)origins & 3) why = "the origin list must be 4-byte aligned";
    if (why) { lg_set_error("scene_gather: %s", why); return -1; }
    SceneGatherArgs a;
    a.pan = pan; a.ms = ms; a.org = origins + 2 * first; a.o_pan = o_pan; a.o_ms = o_ms;
    a.C = C; a.H = H; a.W = W; a.th = th; a.tw = tw;
    a.divisor = divisor; a.post_scale = post_scale; a.n_div = n_div; a.has_scale = post_scale != 1.0f;
    const hipStream_t s = (hipStream_t)stream;
    ProfScope prof(LG_K_SCENE_GATHER, s);
    if (dtype == LG_DT_U8) sg_launch<uint8_t>(a, B, s);
    else if (dtype == LG_DT_U16) sg_launch<uint16_t>(a, B, s);
    else sg_launch<float>(a, B, s);
    LG_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// blend
// ------------------------------------------------------------------------------------------------
// one axis of scene.tile_grid: n tiles of t pixels at origins min(i * s, L - t), s = t - overlap
struct SceneAxis { int L, t, s, n; };

static SceneAxis scene_axis(int L, int t, int overlap) {
    SceneAxis a;
    a.L = L; a.t = t; a.s = t - overlap;
    a.n = L == t ? 1 : (L - t + a.s - 1) / a.s + 1;
    return a;
}
__device__ __forceinline__ int sa_origin(int i, const SceneAxis& a) {
    const int o = i * a.s, m = a.L - a.t;
    return o < m ? o : m;
}
// the tiles lo .. hi that cover pixel p: tiles below the last sit at i * s, the last one flush with the border
__device__ __forceinline__ void sa_cover(int p, const SceneAxis& a, int& lo, int& hi) {
    hi = p >= a.L - a.t ? a.n - 1 : p / a.s;
    lo = p < a.t ? 0 : (p - a.t) / a.s + 1;
    lo = lo < a.n - 1 ? lo : a.n - 1;
}
// w(u) = min(1, (min(u, t - 1 - u) + 1) / (overlap + 1)) as one correctly rounded division of two small integers
__device__ __forceinline__ float sa_weight(int u, int t, int ov1) {
    int k = (u < t - 1 - u ? u : t - 1 - u) + 1;
    k = k < ov1 ? k : ov1;
    return __fdiv_rn((float)k, (float)ov1);
}

__global__ __launch_bounds__(SC_NT) void k_scene_blend(const float* __restrict__ tiles, float* __restrict__ scene, int first, int B, int C,
                                                       const SceneAxis ay, const SceneAxis ax, int ov1) {
    const int qpr = ax.t >> 2;
    const int q = blockIdx.x * SC_NT + threadIdx.x;
    if (q >= ay.t * qpr) return;
    const int c = blockIdx.y, b = blockIdx.z, k = first + b, last = first + B - 1;
    const int ly = q / qpr, lx = (q - ly * qpr) << 2;
    const int iy = k / ax.n, ix = k - iy * ax.n;
    const int y = sa_origin(iy, ay) + ly, x = sa_origin(ix, ax) + lx;
    int ylo, yhi, xlo, xhi;
    sa_cover(y, ay, ylo, yhi);
    sa_cover(x, ax, xlo, xhi);                     // tile boundaries are multiples of 4: pixels x .. x + 3 have the same cover
    float4* sp = reinterpret_cast<float4*>(scene + ((size_t)c * ay.L + y) * ax.L + x);
    const size_t plane = (size_t)ay.t * ax.t;
    if (yhi == ylo && xhi == xlo) {                // covered by this tile alone: a copy
        *sp = *reinterpret_cast<const float4*>(tiles + ((size_t)b * C + c) * plane + (size_t)ly * ax.t + lx);
        return;
    }
    const bool prior = ylo * ax.n + xlo < first;   // an earlier launch left the partial sum of the lower covers in the scene
    const bool closes = yhi * ax.n + xhi <= last;   // the highest cover is in this batch: divide
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    bool have = false;
    for (int jy = ylo; jy <= yhi; ++jy) {
        const int uy = y - sa_origin(jy, ay);
        const float wy = sa_weight(uy, ay.t, ov1);
        for (int jx = xlo; jx <= xhi; ++jx) {
            const int kk = jy * ax.n + jx;
            if (kk < first || kk > last) continue;
            if (!have) {
                if (kk != k) return;               // a lower tile of this batch owns these pixels
                have = true;
                if (prior) { const float4 p = *sp; acc[0] = p.x; acc[1] = p.y; acc[2] = p.z; acc[3] = p.w; }
            }
            const int ux = x - sa_origin(jx, ax);
            const float4 v4 = *reinterpret_cast<const float4*>(tiles + ((size_t)(kk - first) * C + c) * plane + (size_t)uy * ax.t + ux);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
            const bool start = !prior && kk == k;  // the pixel's lowest cover of the whole grid: the chain starts with a product
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float w = __fmul_rn(wy, sa_weight(ux + i, ax.t, ov1));
                acc[i] = start ? __fmul_rn(w, v[i]) : __fmaf_rn(w, v[i], acc[i]);
            }
        }
    }
    if (closes) {
        // the weight sum of ALL covers of the grid: sum_y wy * sum_x wx (the cover set is a product set and the window separable)
        float sy = 0.f;
        for (int jy = ylo; jy <= yhi; ++jy) {
            const float wy = sa_weight(y - sa_origin(jy, ay), ay.t, ov1);
            sy = jy == ylo ? wy : __fadd_rn(sy, wy);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float sx = 0.f;
            for (int jx = xlo; jx <= xhi; ++jx) {
                const float wx = sa_weight(x + i - sa_origin(jx, ax), ax.t, ov1);
                sx = jx == xlo ? wx : __fadd_rn(sx, wx);
            }
            acc[i] = __fdiv_rn(acc[i], __fmul_rn(sy, sx));
        }
    }
    *sp = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

extern "C" int lg_scene_blend(const float* tiles, float* scene, int64_t first, int32_t B, int32_t C, int32_t H, int32_t W, int32_t th, int32_t tw,
                              int32_t overlap, void* stream) {
    const char* why = nullptr;
    if (!tiles || !scene) why = "null pointer";
    else if (B <= 0 || B > 65535) why = "B must be in 1 .. 65535";
    else if ((why = scene_shape_check(C, H, W, th, tw)) != nullptr) {}
    else if (overlap < 0 || (overlap & 3) || 2 * overlap > (th < tw ? th : tw)) why = "the overlap must be a non-negative multiple of 4, at most half the smaller tile side";
    else if (((uintptr_t)tiles | (uintptr_t)scene) & 15) why = "tile and scene arrays must be 16-byte aligned";
    if (!why) {
        const SceneAxis ay = scene_axis(H, th, overlap), ax = scene_axis(W, tw, overlap);
        if (first < 0 || first + B > (int64_t)ay.n * ax.n) why = "tiles first .. first + B - 1 must lie inside the grid";
    }
    if (why) { lg_set_error("scene_blend: %s", why); return -1; }
    const SceneAxis ay = scene_axis(H, th, overlap), ax = scene_axis(W, tw, overlap);
    const hipStream_t s = (hipStream_t)stream;
    ProfScope prof(LG_K_SCENE_BLEND, s);
    k_scene_blend<<<dim3((th * (tw / 4) + SC_NT - 1) / SC_NT, C, B), SC_NT, 0, s>>>(tiles, scene, (int)first, B, C, ay, ax, overlap + 1);
    LG_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// digital numbers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sc_u16(float x, float scale) {
    float r = rintf(__fmul_rn(x, scale));                      // round half to even, like numpy.rint
    r = r > 0.f ? (r < 65535.f ? r : 65535.f) : 0.f;           // NaN -> 0
    return (uint32_t)r;
}
__global__ __launch_bounds__(SC_NT) void k_scene_to_u16(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t quads, float scale) {
    const int64_t q = (int64_t)blockIdx.x * SC_NT + threadIdx.x;
    if (q >= quads) return;
    const float4 v = reinterpret_cast<const float4*>(src)[q];
    reinterpret_cast<uint2*>(dst)[q] = make_uint2(sc_u16(v.x, scale) | (sc_u16(v.y, scale) << 16), sc_u16(v.z, scale) | (sc_u16(v.w, scale) << 16));
}

extern "C" int lg_scene_to_u16(const float* src, uint16_t* dst, int64_t n, float scale, void* stream) {
    const char* why = nullptr;
    if (!src || !dst) why = "null pointer";
    else if (n <= 0 || (n & 3) || n / 4 > (int64_t)0x7fffffff * SC_NT) why = "the sample count must be a positive multiple of 4 below 2^39";
    else if (!(scale == scale) || scale == INFINITY || scale == -INFINITY) why = "the scale must be finite";
    else if (((uintptr_t)src & 15) || ((uintptr_t)dst & 7)) why = "the source must be 16-byte and the destination 8-byte aligned";
    if (why) { lg_set_error("scene_to_u16: %s", why); return -1; }
    const int64_t quads = n / 4;
    k_scene_to_u16<<<(unsigned)((quads + SC_NT - 1) / SC_NT), SC_NT, 0, (hipStream_t)stream>>>(src, dst, quads, scale);
    LG_CHECK_LAUNCH();
    return 0;
}
