// pafuse_hip.hip - host side of the C ABI declared in include/pafuse_hip.h: argument checks, kernel selection
// per width, the MixSTE2 layer schedule and the D3DP DDIM loop.  No allocation, no synchronisation.
#include "../../include/pafuse_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "kernels.hpp"
#include "hgemm.hpp"
#include "xgemm.hpp"
#include "sgemm.hpp"
#include "train_kernels.hpp"

using namespace pafuse;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(PAFUSE_E_HIP, "%s: %s", what, hipGetErrorString(e));
    return PAFUSE_OK;
}

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// "first call on the current device" latch for per-device function attributes (benign race: the guarded call is
// idempotent).  A failing hipGetDevice reports "first" every time, which is merely slower.
struct DeviceOnce {
    static constexpr int MAX_DEV = 64;
    bool done[MAX_DEV] = {};
    bool first() {
        int d = -1;
        if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= MAX_DEV) return true;
        if (done[d]) return false;
        done[d] = true;
        return true;
    }
};

// The one launch stanza.  The kernel is a template argument, so its latch below exists once per kernel instantiation.
// A launch with more than 64 KB of dynamic LDS needs the kernel's ceiling raised first, once per device (one-process
// multi-device callers: nn.DataParallel); `lds_attr` is that ceiling where it is not the launch's own size.
template <auto Kernel> DeviceOnce g_lds_raised;

template <auto Kernel, class... Args>
int launch_lds(const char* name, dim3 grid, unsigned threads, size_t lds, size_t lds_attr, hipStream_t s, const Args&... args) {
    if (lds_attr > 64 * 1024 && g_lds_raised<Kernel>.first()) {
        const hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_attr);
        if (e != hipSuccess) return fail(PAFUSE_E_HIP, "%s: %s", name, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(Kernel, grid, dim3(threads), lds, s, args...);
    return check_launch(name);
}
template <auto Kernel, class... Args>
int launch(const char* name, dim3 grid, unsigned threads, size_t lds, hipStream_t s, const Args&... args) {
    return launch_lds<Kernel>(name, grid, threads, lds, lds, s, args...);
}
inline unsigned blocks_for(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// the grid of a kernel that runs one wave per item, four per workgroup (kernels.hpp wave_item), refused if out of range
int wave_grid(const char* who, int64_t waves, unsigned& grid) {
    if ((waves + 3) / 4 > 0x7fffffff) return fail(PAFUSE_E_ARG, "%s: grid out of range", who);
    grid = blocks_for(waves, 4);
    return PAFUSE_OK;
}

// f(std::integral_constant<int, SLOTS>) for the LaneJoints form that holds J joints: a lane's joints in registers up to
// J = 256 (SLOTS 1 .. 4); beyond, the same arithmetic round by round (SLOTS 0)
template <class F>
int by_joint_slots(int J, F&& f) {
    switch ((J + 63) / 64) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return f(std::integral_constant<int, 0>{});
    }
}

// f(std::integral_constant<int, R>) for a kernel whose lanes keep R = 1 .. 4 items each in registers: count <= 256, which
// the caller has checked
template <class F>
int by_lane_slots(int count, F&& f) {
    switch ((count + 63) / 64) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}

// Makes the device of the caller's stream current for the duration of an entry point (kernel launches, events and
// function attributes go to the CURRENT device): a caller whose tensors live on cuda:1 while cuda:0 is current
// would otherwise record events on the wrong device.  The legacy null stream belongs to the current device.
struct StreamDevice {
    int prev = -1;
    bool switched = false;
    explicit StreamDevice(void* stream) {
        hipDevice_t d = -1;
        if (stream && hipStreamGetDevice((hipStream_t)stream, &d) == hipSuccess && hipGetDevice(&prev) == hipSuccess &&
            d >= 0 && d != prev)
            switched = hipSetDevice(d) == hipSuccess;
        (void)hipGetLastError();  // a failed query must not surface as the next launch's error
    }
    ~StreamDevice() {
        if (switched) (void)hipSetDevice(prev);
    }
    StreamDevice(const StreamDevice&) = delete;
    StreamDevice& operator=(const StreamDevice&) = delete;
};

// ------------------------------------------------------------------------------------------------ GEMM dispatch
template <int WM, int WN, int NT, int EPI, int NSTAGE, int MINW = 1, int TR = 0, int BF16 = 0>
int launch_gemm(const GemmParams& p, hipStream_t s) {
    using T = GemmTile<WM, WN, NT>;
    constexpr size_t stage_bytes = (size_t)NSTAGE * (BF16 == 2 ? T::STAGE_FLOATS_SPLIT : T::STAGE_FLOATS) * sizeof(float);
    if (BF16 == 2 && !p.Wsplit) return fail(PAFUSE_E_ARG, "split-precision GEMM without a pre-split weight image");
    static_assert(EPI == EPI_BIAS || 7 * T::BM * WN <= NSTAGE * T::STAGE_FLOATS, "cross-wave reduction scratch must fit");
    static_assert(stage_bytes <= 160 * 1024, "LDS budget");
    constexpr auto k = gemm_kernel<WM, WN, NT, EPI, NSTAGE, MINW, TR, BF16>;
    const int64_t tiles_m = (p.M + T::BM - 1) / T::BM;
    const int64_t tiles = tiles_m * (p.N / T::BN);
    if (tiles <= 0 || tiles > 0x7fffffff) return fail(PAFUSE_E_ARG, "gemm grid out of range");
#ifdef PAFUSE_DIAG
    static const int dbg_pad = [] { const char* e = getenv("PAFUSE_DEBUG_LDS_PAD"); return e ? atoi(e) : 0; }();
    if (dbg_pad && BF16 == 2 && EPI == EPI_BIAS) {  // diagnostic: keep other kernels off this workgroup's CU (set on every call, as before)
        const size_t lds = std::max(stage_bytes, (size_t)dbg_pad);
        hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k, dim3((unsigned)tiles), dim3(T::NTHR), lds, s, p);
        return check_launch("gemm_kernel");
    }
#endif
    return launch<k>("gemm_kernel", (unsigned)tiles, T::NTHR, stage_bytes, s, p);
}

// qkv projection + attention of one head per workgroup (kernels.hpp fqa_kernel)
template <int LP, int DP>
int launch_fqa(const FqaParams& f, hipStream_t s) {
    using FT = FqaTile<LP, DP>;
    static_assert(FT::LDS_BYTES <= 80 * 1024, "two workgroups per CU");
    const int64_t ntiles = (f.nseq + f.nseq_tile - 1) / f.nseq_tile;
    const int64_t blocks = (ntiles + 7) / 8 * 8 * f.heads;
    if (blocks <= 0 || blocks > 0x7fffffff) return fail(PAFUSE_E_ARG, "fused qkv-attention grid out of range");
    return launch<fqa_kernel<LP, DP>>("fqa_kernel", (unsigned)blocks, 256, FT::LDS_BYTES, s, f);
}

// padded sizes of the fused kernel for a sequence length / head dim, 0 = no fused form (the caller keeps qkv GEMM + attention)
// (the image modes also have an 80-token form on five waves - 160-row tiles - for head dim <= 32: the face's 68 joints)
static int fqa_lp(int L, int mode) { return L <= 32 ? 32 : (L <= 48 ? 48 : (mode_images(mode) && L <= 80 ? 80 : 0)); }
static int fqa_dp(int d) { return (d % 4 || d > 48) ? 0 : (d <= 32 ? 32 : 48); }
static bool fqa_has(int L, int d, int mode) {   // (48, 48) would need 80.4 KB of LDS: one workgroup per CU, not built
    const int lp = fqa_lp(L, mode), dp = fqa_dp(d);
    return lp && dp && !(lp >= 48 && dp == 48);
}
// mode 4 (xgemm.hpp xfqa_kernel): the workgroup's columns come in whole 32-column blocks - two heads at head dim 33 .. 48
static bool xfqa_has(int L, int d, int heads) { return fqa_has(L, d, MODE_BF16X3_IMAGES) && (fqa_dp(d) == 32 || heads % 2 == 0); }
// rows of the fused kernel's q | k | v tiles, and whole sequences per tile (the last one's LP-row key tile inside the buffer)
static int fqa_rows(int lp) { return lp == 80 ? 160 : 128 + (lp == 48 ? 4 : 0); }
static int fqa_tile_rows(int lp) { return lp == 80 ? 160 : 128; }
static int fqa_nseq_tile(int L, int lp) { return (fqa_rows(lp) - lp) / L + 1; }

// the same decomposition in the f16x2 H pipeline (hgemm.hpp hfqa_kernel): A and the head-major weight as H images, o as H image
template <int LP, int DP, int HPW>
int launch_hfqa(const FqaParams& f, hipStream_t s) {
    using FT = HfqaTile<LP, DP, HPW>;
    static_assert(FT::LDS_BYTES <= 80 * 1024, "two workgroups per CU");
    if (f.heads % HPW) return fail(PAFUSE_E_SHAPE, "fused qkv-attention: %d heads do not split into groups of %d", f.heads, HPW);
    if (!f.g.Ah || !f.g.Wh) return fail(PAFUSE_E_ARG, "fused qkv-attention (f16x2) without the H images of its operands");
    if (f.g.M >= (int64_t)1 << 31 || f.nseq >= (int64_t)1 << 31) return fail(PAFUSE_E_ARG, "fused qkv-attention: more than 2^31 tokens");
    const int64_t ntiles = (f.nseq + f.nseq_tile - 1) / f.nseq_tile;
    const int64_t blocks = (ntiles + 7) / 8 * 8 * (f.heads / HPW);
    if (blocks <= 0 || blocks > 0x7fffffff) return fail(PAFUSE_E_ARG, "fused qkv-attention grid out of range");
    return launch<hfqa_kernel<LP, DP, HPW>>("hfqa_kernel", (unsigned)blocks, FT::NTHR, FT::LDS_BYTES, s, f);
}

// ... and in the bf16x3 X pipeline (xgemm.hpp xfqa_kernel): A and the head-major weight as X images, o as X image
template <int LP, int DP, int HPW>
int launch_xfqa(const FqaParams& f, hipStream_t s) {
    using FT = XfqaTile<LP, DP, HPW>;
    static_assert(2 * FT::LDS_BYTES <= 160 * 1024, "two workgroups per CU");
    if (f.heads % HPW) return fail(PAFUSE_E_SHAPE, "fused qkv-attention: %d heads do not split into groups of %d", f.heads, HPW);
    if (!f.g.Ah || !f.g.Wh) return fail(PAFUSE_E_ARG, "fused qkv-attention (bf16x3 images) without the X images of its operands");
    if (f.g.K % 32 || f.g.K <= 0) return fail(PAFUSE_E_SHAPE, "fused qkv-attention: K=%d must be a positive multiple of 32", f.g.K);
    if (f.g.M >= (int64_t)1 << 31 || f.nseq >= (int64_t)1 << 31) return fail(PAFUSE_E_ARG, "fused qkv-attention: more than 2^31 tokens");
    const int64_t ntiles = (f.nseq + f.nseq_tile - 1) / f.nseq_tile;
    const int64_t blocks = (ntiles + 7) / 8 * 8 * (f.heads / HPW);
    if (blocks <= 0 || blocks > 0x7fffffff) return fail(PAFUSE_E_ARG, "fused qkv-attention grid out of range");
    return launch<xfqa_kernel<LP, DP, HPW>>("xfqa_kernel", (unsigned)blocks, FT::NTHR, FT::LDS_BYTES, s, f);
}

int fused_qkv_attention(const FqaParams& f, hipStream_t s) {
    if (f.nseq <= 0) return PAFUSE_OK;
    const int lp = fqa_lp(f.L, f.g.mode), dp = fqa_dp(f.d);
    if (f.g.mode == MODE_BF16X3_IMAGES) {
        if (lp == 80 && dp == 32) return launch_xfqa<80, 32, 1>(f, s);
        if (lp == 32 && dp == 48) return launch_xfqa<32, 48, 2>(f, s);
        if (lp == 32 && dp == 32) return f.heads % 2 ? launch_xfqa<32, 32, 1>(f, s) : launch_xfqa<32, 32, 2>(f, s);
        if (lp == 48 && dp == 32) return f.heads % 2 ? launch_xfqa<48, 32, 1>(f, s) : launch_xfqa<48, 32, 2>(f, s);
        return fail(PAFUSE_E_SHAPE, "fused qkv-attention: no kernel for L=%d, d=%d", f.L, f.d);
    }
    if (f.g.mode == MODE_F16X2) {
        if (lp == 80 && dp == 32) return launch_hfqa<80, 32, 1>(f, s);
        // head dim <= 32: two heads per workgroup share the A stream (the ring grows to the 80 KB two workgroups per CU allow)
        if (lp == 32 && dp == 48) return launch_hfqa<32, 48, 1>(f, s);
        if (lp == 32 && dp == 32) return f.heads % 2 ? launch_hfqa<32, 32, 1>(f, s) : launch_hfqa<32, 32, 2>(f, s);
        if (lp == 48 && dp == 32) return f.heads % 2 ? launch_hfqa<48, 32, 1>(f, s) : launch_hfqa<48, 32, 2>(f, s);
        return fail(PAFUSE_E_SHAPE, "fused qkv-attention: no kernel for L=%d, d=%d", f.L, f.d);
    }
    if (lp == 32 && dp == 48) return launch_fqa<32, 48>(f, s);
    if (lp == 32 && dp == 32) return launch_fqa<32, 32>(f, s);
    if (lp == 48 && dp == 32) return launch_fqa<48, 32>(f, s);
    return fail(PAFUSE_E_SHAPE, "fused qkv-attention: no kernel for L=%d, d=%d", f.L, f.d);
}

// fc1 -> GELU -> fc2 -> whole-row epilogue in one kernel (hgemm.hpp hmlp_kernel): f16x2, folded LayerNorm, H-image residual only
static bool hmlp_has(int C, int hidden) { return hidden == 2 * C && (C == 224 || C == 256 || C == 384); }
template <int NT2, int MINW>
int launch_hmlp(const MlpParams& m, hipStream_t s) {
    using T = MlpTile<NT2>;
    static_assert(T::LDS_BYTES <= (MINW == 2 ? 80 : 160) * 1024, "LDS budget");
    const int64_t tiles = (m.g.M + 127) / 128;
    if (tiles <= 0 || tiles > 0x7fffffff) return fail(PAFUSE_E_ARG, "fused MLP grid out of range");
    return launch<hmlp_kernel<NT2, MINW>>("hmlp_kernel", (unsigned)tiles, 256, T::LDS_BYTES, s, m);   // 74 - 75 KB
}
int fused_mlp(const MlpParams& m, hipStream_t s) {
    if (m.g.M <= 0) return PAFUSE_OK;
    if (!m.g.Ah || !m.g.Wh || !m.W1h || !m.bias1 || !m.g.resid_h) return fail(PAFUSE_E_ARG, "fused MLP without its H images");
    if (m.g.K != 2 * m.g.N) return fail(PAFUSE_E_SHAPE, "fused MLP: hidden width %d is not twice the channel width %d", m.g.K, m.g.N);
    switch (m.g.N) {
        case 224: return launch_hmlp<7, 2>(m, s);
        case 256: return launch_hmlp<8, 2>(m, s);
        case 384: return launch_hmlp<12, 1>(m, s);
        default: return fail(PAFUSE_E_SHAPE, "fused MLP: no kernel for channel width %d", m.g.N);
    }
}

// the qkv layers' kernel on v_mfma_f32_16x16x32_bf16 (kernels.hpp gemm16_tile); the image must be in the M16 layout
template <int NB, int MINW>
int launch_gemm16(const GemmParams& p, hipStream_t s) {
    using T = Tile16<NB>;
    static_assert(T::STAGE_BYTES <= 64 * 1024, "LDS budget without the attribute");
    if (!p.Wsplit) return fail(PAFUSE_E_ARG, "split-precision GEMM without a pre-split weight image");
    const int64_t tiles = ((p.M + T::BM - 1) / T::BM) * (p.N / T::BN);
    if (tiles <= 0 || tiles > 0x7fffffff) return fail(PAFUSE_E_ARG, "gemm grid out of range");
    return launch<gemm16_kernel<NB, MINW>>("gemm16_kernel", (unsigned)tiles, T::NTHR, T::STAGE_BYTES, s, p);
}

// ---- the strip GEMM (sgemm.hpp, round 6): the plain split-precision layers (qkv, fc1) on the software-pipelined persistent kernel.
// A launch is STRIP_WGS_PER_CU workgroups per CU (two fit: 68 - 80 KB of LDS each) walking the tile stream; fewer tiles than slots
// = one workgroup per tile.  The CU count is the current device's (cached per device).
#ifndef PAFUSE_STRIP_WGS_PER_CU
#define PAFUSE_STRIP_WGS_PER_CU 2
#endif
int device_cus() {
    static int cus[DeviceOnce::MAX_DEV] = {};
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= DeviceOnce::MAX_DEV) return 256;
    if (!cus[d]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n <= 0) n = 256;
        cus[d] = n;
    }
    return cus[d];
}

template <int NB, int FLAGS>
int launch_strip2(const GemmParams& p, hipStream_t s) {
    constexpr int RG = 2, NW = 4;
    using T = StripTile<NB, RG, NW, 2>;
    static_assert(T::LDS_BYTES <= 80 * 1024, "two workgroups per CU");
    if (!p.Wsplit) return fail(PAFUSE_E_ARG, "split-precision GEMM without a pre-split weight image");
    const int64_t tiles = ((p.M + T::BM - 1) / T::BM) * (p.N / T::BN);
    if (tiles <= 0 || tiles > 0x7fffffff) return fail(PAFUSE_E_ARG, "gemm grid out of range");
    int64_t grid = (int64_t)device_cus() * PAFUSE_STRIP_WGS_PER_CU / 8 * 8;   // a multiple of 8: virtual workgroup v = b + j grid keeps b's XCD
    if (grid >= tiles || grid <= 0) grid = tiles;
    return launch<sgemm2_kernel<NB, RG, NW, SEPI_BIAS, 2, FLAGS>>("sgemm2_kernel", (unsigned)grid, T::NTHR, T::LDS_BYTES, s, p);
}
// which plain layers the strip kernel takes: an M16 image, at most one training epilogue option (alone), at least four 32-deep chunks (the deferred
// stores of a tile go out inside the first four chunks of the next one), a column count one of its tiles divides
bool strip2_ok(const GemmParams& p) {
    if ((p.out_act || p.dact_u) && (p.ln_in || p.act || (p.out_act && p.dact_u))) return false;   // training options: alone, on a plain product
    return p.mode == MODE_BF16X3 && p.wlayout == WLAYOUT_M16 && p.K % 32 == 0 && p.K >= 128 && p.M > 0 &&
           p.M * (int64_t)p.N < (int64_t)1 << 31 && p.M * (int64_t)p.K < (int64_t)1 << 31 &&   // (32-bit float offsets of its rows)
           (p.N % 128 == 0 || p.N % 112 == 0 || p.N % 96 == 0);
}
template <int NB>
int launch_strip2_flags(const GemmParams& p, hipStream_t s) {
    const int flags = (p.ln_in ? 1 : 0) | (p.act ? 2 : 0) | (p.dact_u ? 4 : 0) | (p.out_act ? 8 : 0);
    switch (flags) {
        case 0: return launch_strip2<NB, 0>(p, s);
        case 1: return launch_strip2<NB, 1>(p, s);
        case 2: return launch_strip2<NB, 2>(p, s);
        case 3: return launch_strip2<NB, 3>(p, s);
        case 4: return launch_strip2<NB, 4>(p, s);   // training: dX of fc2
        case 8: return launch_strip2<NB, 8>(p, s);   // training: fc1 forward
        default: return fail(PAFUSE_E_ARG, "strip GEMM: epilogue options %d", flags);
    }
}
int strip2_bias(const GemmParams& p, hipStream_t s) {
    if (p.N % 128 == 0) return launch_strip2_flags<8>(p, s);    // body 1152 / 768, hands 768 / 512: 128 x 128
    if (p.N % 112 == 0) return launch_strip2_flags<7>(p, s);    // face 672 / 448: 128 x 112
    return launch_strip2_flags<6>(p, s);                         // 128 x 96 (the single-model variant: 864 = 9 x 96)
}

// split-precision GEMM, LDS-DMA pipelined form (one workgroup per CU, NSTAGE ring of 32-deep chunks)
// K-chunk depth of the pre-split image of a weight (the image format is a property of the weight, fixed when it is
// split, so every launch on it - any M - must use a kernel of that depth): the whole-row layers of widths 384, 288, 256
// and 224 run on the LDS-DMA kernel with 16-deep chunks, everything else on 32-deep chunks.
int wsplit_chunk(int N, bool whole_row) { return (whole_row && (N == 384 || N == 288 || N == 256 || N == 224)) ? 16 : 32; }

template <int WM, int WN, int NT, int EPI, int NSTAGE, int MINW, int BKC = 32>
int launch_gemm_dma(const GemmParams& p, hipStream_t s) {
    using T = DmaTile<WM, WN, NT, BKC>;
    constexpr size_t lds = (size_t)NSTAGE * T::STAGE_BYTES;
    static_assert(lds <= 160 * 1024, "LDS budget");
    static_assert(EPI == EPI_BIAS || (size_t)7 * T::BM * WN * sizeof(float) <= lds, "cross-wave reduction scratch must fit");
    if (!p.Wsplit) return fail(PAFUSE_E_ARG, "split-precision GEMM without a pre-split weight image");
    if (p.K % BKC) return fail(PAFUSE_E_SHAPE, "split GEMM: K=%d is not a multiple of %d", p.K, BKC);
    const int64_t tiles = (p.M + T::BM - 1) / T::BM * (p.N / T::BN);
    if (tiles <= 0 || tiles > 0x7fffffff) return fail(PAFUSE_E_ARG, "gemm grid out of range");
    return launch<gemm_dma_kernel<WM, WN, NT, EPI, NSTAGE, MINW, 0, BKC>>("gemm_dma_kernel", (unsigned)tiles, T::NTHR, lds, s, p);
}

// ---- f16x2 "H pipeline" (hgemm.hpp): both operands arrive as H images; one workgroup of WM x WN waves per CU
template <int WM, int WN, int NT, int EPI, int NSTAGE, int BKC, int MINW, bool HRES = false>
int launch_hgemm(const GemmParams& p, hipStream_t s) {
    using T = HTile<WM, WN, NT, BKC>;
    constexpr size_t lds = (size_t)NSTAGE * T::STAGE_BYTES;
    static_assert(lds <= 160 * 1024, "LDS budget");
    static_assert(EPI == EPI_BIAS || (size_t)7 * T::BM * WN * sizeof(float) <= lds, "cross-wave reduction scratch must fit");
    if (!p.Ah || !p.Wh) return fail(PAFUSE_E_ARG, "f16x2 GEMM without the H images of its operands");
    if (p.K % BKC || p.K <= 0 || p.N % T::BN) return fail(PAFUSE_E_SHAPE, "f16x2 GEMM: N=%d, K=%d do not fit the %d-column tile", p.N, p.K, T::BN);
    if (HRES && !p.resid_h) return fail(PAFUSE_E_ARG, "f16x2 whole-row GEMM: no H-image residual");
    const int64_t tiles = (p.M + T::BM - 1) / T::BM * (p.N / T::BN);
    if (tiles <= 0 || tiles > 0x7fffffff) return fail(PAFUSE_E_ARG, "gemm grid out of range");
    return launch<hgemm_kernel<WM, WN, NT, EPI, NSTAGE, BKC, MINW, HRES>>("hgemm_kernel", (unsigned)tiles, T::NTHR, lds, s, p);
}

// widths the f16x2 kernels serve: the PAFUSE parts' (whole-row layers), and every plain-layer width that tiles by 128 or 224
bool hgemm_width(int C) { return C == 384 || C == 256 || C == 224; }
bool hgemm_plain_n(int N) { return N > 0 && (N % 128 == 0 || N % 224 == 0); }

// tile choice per shape: tools/hgemm_bench.hip (profiles/r04_hgemm_bench_*.log).  With three products per k these layers sit
// between the matrix, the L2 -> LDS and the HBM bound (a whole-row launch moves 4 M C floats for 6 M C K MFMA-flops), so the
// winners are the tiles that keep MORE workgroups per CU in different phases, not the tallest ones.
int hgemm_bias(const GemmParams& p, hipStream_t s) {
    if (p.M <= 0) return PAFUSE_OK;
    if (p.N % 128 == 0) return launch_hgemm<4, 2, 2, EPI_BIAS, 3, 16, 2>(p, s);   // 128 x 128, eight waves, three per CU
    if (p.N % 224 == 0) return launch_hgemm<4, 1, 7, EPI_BIAS, 3, 16, 2>(p, s);   // 128 x 224 (the face: 672 = 3 x 224, 448 = 2 x 224)
    return fail(PAFUSE_E_SHAPE, "f16x2 linear: N=%d must be a multiple of 128 or 224", p.N);
}

int hgemm_rowln(const GemmParams& p, hipStream_t s) {
    if (p.M <= 0) return PAFUSE_OK;
    if (p.resid_h)   // the residual stream as its (centred) H image: the default of the folded-LayerNorm pipeline
        switch (p.N) {
            case 384: return launch_hgemm<4, 2, 6, EPI_ROWLN, 2, 32, 1, true>(p, s);
            case 256: return launch_hgemm<2, 2, 4, EPI_ROWLN, 2, 32, 2, true>(p, s);
            case 224: return launch_hgemm<4, 1, 7, EPI_ROWLN, 3, 16, 2, true>(p, s);
            default: break;
        }
    switch (p.N) {
        case 384: return launch_hgemm<4, 2, 6, EPI_ROWLN, 2, 32, 1>(p, s);   // 128 rows, eight waves, 128 KB ring: one per CU
        case 256: return launch_hgemm<2, 2, 4, EPI_ROWLN, 2, 32, 2>(p, s);   // 64 rows, four waves, 32-deep chunks, two per CU
        case 224: return launch_hgemm<4, 1, 7, EPI_ROWLN, 3, 16, 2>(p, s);   // 128 rows, four waves (7 column blocks do not split), two per CU
        default: return fail(PAFUSE_E_SHAPE, "no f16x2 whole-row kernel for channel width %d (have 224, 256, 384)", p.N);
    }
}

// ---- bf16x3 "X pipeline" (xgemm.hpp): both operands arrive as X images
template <int WM, int WN, int NT, int EPI, int NSTAGE, int BKC, int MINW, bool HRES = false>
int launch_xgemm(const GemmParams& p, hipStream_t s) {
    using T = XTile<WM, WN, NT, BKC>;
    constexpr size_t lds = (size_t)NSTAGE * T::STAGE_BYTES;
    static_assert(lds <= 160 * 1024, "LDS budget");
    static_assert(EPI == EPI_BIAS || (size_t)7 * T::BM * WN * sizeof(float) <= lds, "cross-wave reduction scratch must fit");
    if (!p.Ah || !p.Wh) return fail(PAFUSE_E_ARG, "bf16x3 image GEMM without the X images of its operands");
    if (p.K % 32 || p.K <= 0 || p.N % T::BN) return fail(PAFUSE_E_SHAPE, "bf16x3 image GEMM: N=%d, K=%d do not fit the %d-column tile", p.N, p.K, T::BN);
    if (HRES && !p.resid_h) return fail(PAFUSE_E_ARG, "bf16x3 whole-row GEMM: no X-image residual");
    const int64_t tiles = (p.M + T::BM - 1) / T::BM * (p.N / T::BN);
    if (tiles <= 0 || tiles > 0x7fffffff) return fail(PAFUSE_E_ARG, "gemm grid out of range");
    return launch<xgemm_kernel<WM, WN, NT, EPI, NSTAGE, BKC, MINW, HRES>>("xgemm_kernel", (unsigned)tiles, T::NTHR, lds, s, p);
}

// tile choice per shape: tools/xgemm_bench.hip (profiles/r05_xgemm_bench.log).  With six products per k the K loops of these
// tiles are balanced between the matrix pipe and the L2 -> LDS stream (a 128 x 128 tile asks for 24 KB per 768 matrix cycles,
// the stream gives 25 - 32 B per cycle and CU; in-kernel stamps: 70 - 80 % matrix-pipe use inside the loops).  What is left is per
// tile - first-chunk latency, epilogue, the last partial round of a launch -, so the winners are the tiles that keep MORE
// workgroups per CU in different phases (four-wave tiles on two-stage rings of 16-deep chunks: three per CU).
int xgemm_bias(const GemmParams& p, hipStream_t s) {
    if (p.M <= 0) return PAFUSE_OK;
    if (p.N % 128 == 0) return launch_xgemm<4, 1, 4, EPI_BIAS, 2, 16, 3>(p, s);   // 128 x 128, four waves, 48 KB ring: three per CU
    if (p.N % 224 == 0) return launch_xgemm<4, 1, 7, EPI_BIAS, 2, 16, 2>(p, s);   // 128 x 224 (the face: 448 = 2 x 224), 66 KB: two per CU
    if (p.N % 96 == 0) return launch_xgemm<4, 1, 3, EPI_BIAS, 3, 16, 2>(p, s);    // 128 x 96 (unit tests: 672, 96)
    return fail(PAFUSE_E_SHAPE, "bf16x3 image linear: N=%d must be a multiple of 128, 224 or 96", p.N);
}

int xgemm_rowln(const GemmParams& p, hipStream_t s) {
    if (p.M <= 0) return PAFUSE_OK;
    if (p.resid_h)   // the residual stream as its (centred) X image: the default of the folded-LayerNorm pipeline
        switch (p.N) {
            case 384: return launch_xgemm<4, 2, 6, EPI_ROWLN, 3, 16, 1, true>(p, s);   // 128 rows, eight waves, 144 KB ring: one per CU
            case 256: return launch_xgemm<3, 2, 4, EPI_ROWLN, 3, 16, 1, true>(p, s);   // 96 rows, six waves, 99 KB: one per CU (473 tiles: 1.85 rounds)
            case 224: return p.K <= 256 ? launch_xgemm<3, 1, 7, EPI_ROWLN, 2, 16, 2, true>(p, s)     // proj: 96 rows, three waves, 60 KB: two per CU
                                        : launch_xgemm<3, 1, 7, EPI_ROWLN, 3, 16, 2, true>(p, s);    // fc2 (K = 448): a three-stage ring, one per CU
            default: break;
        }
    switch (p.N) {
        case 384: return launch_xgemm<4, 2, 6, EPI_ROWLN, 3, 16, 1>(p, s);
        case 256: return launch_xgemm<2, 2, 4, EPI_ROWLN, 2, 16, 2>(p, s);
        case 224: return launch_xgemm<4, 1, 7, EPI_ROWLN, 2, 16, 2>(p, s);
        default: return fail(PAFUSE_E_SHAPE, "no bf16x3 image whole-row kernel for channel width %d (have 224, 256, 384)", p.N);
    }
}

// diagnostic switch, compiled only into -DPAFUSE_DIAG builds (tools/): environment PAFUSE_DEBUG_F32_MASK, read once -
// bit 0 = plain linear layers, bit 1 = whole-row layers fall back to the fp32 matrix cores even in split-precision mode.
// The shipped library reads no environment variable: nothing outside its arguments changes which kernels it runs.
#ifdef PAFUSE_DIAG
int debug_f32_mask() {
    static const int mask = [] {
        const char* e = getenv("PAFUSE_DEBUG_F32_MASK");
        return e ? atoi(e) : 0;
    }();
    return mask;
}
#else
constexpr int debug_f32_mask() { return 0; }
#endif

// A/B build switch (tools/build_variant.py): workgroups per CU the 128 x 128 plain split tile is compiled for.  3 fits (152
// registers, 43 KB of LDS) and measured slower: 98.5 - 100.2 us per fc1 launch against 95.7 - 97.3 at 2 (round 5, same GPU call).
#ifndef PAFUSE_FC1_MINW
#define PAFUSE_FC1_MINW 2
#endif
int gemm_bias(const GemmParams& p0, hipStream_t s) {
    GemmParams p = p0;
    if (p.mode == MODE_BF16X3 && (debug_f32_mask() & 1)) p.mode = MODE_F32;
    if (p.mode == MODE_BF16X3 && (debug_f32_mask() & 4) && !p.act) p.mode = MODE_F32;   // qkv only
    if (p.mode == MODE_BF16X3 && (debug_f32_mask() & 8) && p.act) p.mode = MODE_F32;    // fc1 only
    if (p.mode == MODE_BF16X3 && (debug_f32_mask() & 16)) {                        // split arithmetic, small 128x64 tiles only
        if (p.N % 64 == 0) return launch_gemm<4, 1, 2, EPI_BIAS, 1, 4, 0, 2>(p, s);
    }
    if (p.M <= 0) return PAFUSE_OK;
    if (p.K % BK || p.N % 32 || p.K <= 0 || p.N <= 0)
        return fail(PAFUSE_E_SHAPE, "linear: N=%d K=%d must be positive multiples of 32", p.N, p.K);
    // the training epilogue options live in the slab epilogue of gemm_tile (every N % 64 == 0 route below ends there) and in gemm16_tile's
    if ((p.out_act || p.dact_u) && ((p.N % 64 && !(p.mode == MODE_BF16X3 && p.wlayout == WLAYOUT_M16)) || mode_images(p.mode) || p.ln_in || p.act))
        return fail(PAFUSE_E_ARG, "linear: out_act / dact_u need N %% 64 == 0 and a plain fp32 or bf16x3 product");
    if (p.mode == MODE_F16X2) return hgemm_bias(p, s);   // f16x2: the H pipeline
    if (p.mode == MODE_BF16X3_IMAGES) return xgemm_bias(p, s);   // bf16x3 on images: the X pipeline
    // small accumulators + single LDS stage = 4-5 independent workgroups per CU, which hides the per-tile
    // prologue/epilogue (measured with tools/gemm_bench.hip: 128x64 tiles reach 72-74 % of the f32 MFMA peak at the
    // qkv shape, 128x96/double-buffered 65-67 %, 128x128 58-60 %)
#ifdef PAFUSE_QKV_32X32   // A/B build (tools/): the qkv layers on the 32x32x16 tiles, their images in layout 0
    p.wlayout = WLAYOUT_PLAIN;
#endif
#ifndef PAFUSE_NO_STRIP
    if (strip2_ok(p)) return strip2_bias(p, s);   // qkv, fc1 (+ GELU): the pipelined persistent strip kernel (sgemm.hpp; same bits as gemm16_tile)
#endif
    if (p.mode == MODE_BF16X3 && p.wlayout == WLAYOUT_M16) {  // 16x16x32 MFMAs on the M16 image (kernels.hpp gemm16_tile): training's epilogue options, short K
        if (p.N % 128 == 0) return launch_gemm16<8, 3>(p, s);    // body 1152, hands 768: 128 x 128 tiles, 3 workgroups per CU
        if (p.N % 96 == 0) return launch_gemm16<6, 3>(p, s);     // face 672, single-model 864: 128 x 96
        if (p.N % 112 == 0) return launch_gemm16<7, 3>(p, s);    // face 224, 448 (training: every plain GEMM of the face): 128 x 112
        if (p.N % 64 == 0) return launch_gemm16<4, 4>(p, s);
        return launch_gemm16<2, 4>(p, s);
    }
    if (p.mode == MODE_BF16X3) {  // split precision (bf16x3): fp32-equivalent products on the bf16 matrix cores
        // measured per shape with tools/gemm_bench.hip (profiles/r02_gemm_bench_split_v1.log): 128x128 tiles at two
        // workgroups per CU where N allows (159 TFLOP/s at the body qkv shape), 128x64 at four otherwise (148)
        if (p.N % 128 == 0 && p.M >= 4096) return launch_gemm<4, 1, 4, EPI_BIAS, 1, PAFUSE_FC1_MINW, 0, 2>(p, s);
        if (p.N % 64 == 0) return launch_gemm<4, 1, 2, EPI_BIAS, 1, 4, 0, 2>(p, s);
        if (p.N % 96 == 0) return launch_gemm<4, 1, 3, EPI_BIAS, 1, 1, 1, 2>(p, s);
        return launch_gemm<4, 1, 1, EPI_BIAS, 1, 1, 0, 2>(p, s);
    }
    if (p.mode != MODE_F32) {  // opt-in bf16-operand mode: same tiles, bf16 MFMA
        if (p.N % 64 == 0) return launch_gemm<4, 1, 2, EPI_BIAS, 1, 5, 0, 1>(p, s);
        if (p.N % 96 == 0) return launch_gemm<4, 1, 3, EPI_BIAS, 1, 1, 1, 1>(p, s);
        return launch_gemm<4, 1, 1, EPI_BIAS, 1, 1, 0, 1>(p, s);
    }
    if (p.N % 64 == 0) return launch_gemm<4, 1, 2, EPI_BIAS, 1, 5>(p, s);   // pin 5 waves/SIMD (98 registers)
    if (p.N % 96 == 0) return launch_gemm<4, 1, 3, EPI_BIAS, 1, 1, 1>(p, s);  // row-per-lane epilogue wins at NT=3
    return launch_gemm<4, 1, 1, EPI_BIAS, 1>(p, s);
}

template <int EPI>
int gemm_rowln_as(const GemmParams& p0, hipStream_t s) {
    GemmParams p = p0;
    if (p.mode == MODE_BF16X3 && (debug_f32_mask() & 2)) p.mode = MODE_F32;
    if (p.M <= 0) return PAFUSE_OK;
    if (p.K % BK || p.K <= 0) return fail(PAFUSE_E_SHAPE, "rowln: K=%d must be a positive multiple of 32", p.K);
    if (p.mode == MODE_F16X2 || p.mode == MODE_BF16X3_IMAGES) {   // f16x2: the H pipeline; bf16x3 on images: the X pipeline (inference only)
        if constexpr (EPI == EPI_ROWLN) return p.mode == MODE_F16X2 ? hgemm_rowln(p, s) : xgemm_rowln(p, s);
        else return fail(PAFUSE_E_ARG, "training has no image-pipeline kernels");
    }
    if constexpr (EPI == EPI_ROWLN_TRAIN) {   // training forward with split products: the three PAFUSE widths (train_host.inc)
        if (p.mode == MODE_BF16X3) {
            switch (p.N) {
                case 384: return launch_gemm_dma<2, 2, 6, EPI, 2, 2, 16>(p, s);
                case 256: return launch_gemm_dma<2, 2, 4, EPI, 2, 2, 16>(p, s);
                case 224: if (p.M >= 4096) return launch_gemm_dma<4, 1, 7, EPI, 2, 2, 16>(p, s); break;
                default: break;
            }
            p.mode = MODE_F32;   // no split whole-row tile for this shape: the fp32 kernels below
        }
    }
    if constexpr (EPI == EPI_ROWLN) {
        if (p.mode == MODE_BF16X3) {
            switch (p.N) {
                // picked per width with tools/gemm_bench.hip (profiles/r02_gemm_bench_*.log): the LDS-DMA kernel on 16-deep
                // chunks, four waves, a two-stage ring and TWO workgroups per CU - the LayerNorm epilogue of one tile
                // (a third of a tile's time when nothing overlaps it) runs under the K loop of the other.  The same
                // variants serve the grouped launches below, so both routes give bit-identical rows.
                // (round 5, with the slab epilogue: 128-row eight-wave tiles - half the weight re-reads - measured again: proj 62 vs 58 us,
                // fc2 104 vs 98: the two-workgroup tiles stay)
                case 384: return launch_gemm_dma<2, 2, 6, EPI, 2, 2, 16>(p, s);
                case 256: return launch_gemm_dma<2, 2, 4, EPI, 2, 2, 16>(p, s);
                case 288: return launch_gemm_dma<2, 3, 3, EPI, 2, 2, 16>(p, s);  // the single-model variant (cs = 288)
                case 224:
                    return p.M >= 4096 ? launch_gemm_dma<4, 1, 7, EPI, 2, 2, 16>(p, s) : launch_gemm_dma<2, 1, 7, EPI, 2, 2, 16>(p, s);
                case 128: return launch_gemm<1, 4, 1, EPI, 1, 1, 1, 2>(p, s);
                case 64: return launch_gemm<1, 2, 1, EPI, 1, 1, 1, 2>(p, s);
                default: break;
            }
        } else if (p.mode != MODE_F32) {
            switch (p.N) {
                case 384: return launch_gemm<1, 4, 3, EPI, 1, 1, 1, 1>(p, s);
                case 288: return launch_gemm<1, 3, 3, EPI, 1, 1, 1, 1>(p, s);
                case 256: return launch_gemm<2, 2, 4, EPI, 1, 2, 1, 1>(p, s);
                case 224: return launch_gemm<1, 7, 1, EPI, 1, 1, 1, 1>(p, s);
                case 128: return launch_gemm<1, 4, 1, EPI, 1, 1, 1, 1>(p, s);
                case 64: return launch_gemm<1, 2, 1, EPI, 1, 1, 1, 1>(p, s);
                default: break;
            }
        }
    }
    switch (p.N) {
        // row-per-lane accumulators (TR): LayerNorm statistics are in-lane sums + one shuffle + a tiny cross-wave
        // exchange, all global traffic is dwordx4, no LDS transposition (picked with tools/gemm_bench.hip)
        case 384: return launch_gemm<1, 4, 3, EPI, 1, 1, 1>(p, s);
        case 288: return launch_gemm<1, 3, 3, EPI, 1, 1, 1>(p, s);
        case 256: return launch_gemm<2, 2, 4, EPI, 1, 2, 1>(p, s);  // (MINW 3 capped it at 168 VGPRs: 6 spilled, -2 %)
        case 224: return launch_gemm<1, 7, 1, EPI, 1, 1, 1>(p, s);
        case 128: return launch_gemm<1, 4, 1, EPI, 1, 1, 1>(p, s);
        case 64: return launch_gemm<1, 2, 1, EPI, 1, 1, 1>(p, s);
        default: return fail(PAFUSE_E_SHAPE, "no whole-row kernel for channel width %d (have 64,128,224,256,288,384)", p.N);
    }
}

int gemm_rowln(const GemmParams& p, hipStream_t s) { return gemm_rowln_as<EPI_ROWLN>(p, s); }
// training forward: the same kernels with the DropPath row factor and the pre-norm sum as an extra output
int gemm_rowln_train(const GemmParams& p, hipStream_t s) { return gemm_rowln_as<EPI_ROWLN_TRAIN>(p, s); }

// ---- grouped launches: the same layer of several independent parts in one grid (kernels.hpp, grouped_*_kernel).
// Only the split-precision mode has them (the fp32 mode overlaps parts on streams instead); anything a grouped kernel
// has no variant for goes part by part through the dispatch above - same tiles, same arithmetic, same results.
bool group_ok_rowln(const GemmParams& p) {
    return p.mode == MODE_BF16X3 && p.Wsplit && (p.N == 384 || p.N == 256 || (p.N == 224 && p.M >= 4096)) && p.K % 16 == 0 && p.K > 0 &&
           !(debug_f32_mask() & 2);
}
// (the plain layers - qkv, fc1 - have no shared grid since round 6: the persistent strip kernel fills the chip from one part's tiles;
// grouped_bias_kernel, the shared 32x32x16 grid of rounds 3 - 5, is gone)
// (whether the parts of a configuration share grids is the caller's choice per call: pafuse_d3dp_config.part_by_part_launches -
// same tiles, same arithmetic, same bits either way; there is no process-wide schedule state)

template <bool ROWLN>
int gemm_group(const GemmParams* ps, int n, hipStream_t s, bool shared_grids) {
    bool ok = ROWLN && shared_grids && n >= 2 && n <= GROUP_MAX;
    for (int i = 0; i < n && ok; ++i) ok = ps[i].M > 0 && group_ok_rowln(ps[i]);
    if (!ok) {
        for (int i = 0; i < n; ++i) {
            const int rc = ROWLN ? gemm_rowln(ps[i], s) : gemm_bias(ps[i], s);
            if (rc) return rc;
        }
        return PAFUSE_OK;
    }
    // most expensive tiles first (the tail of the grid is then made of the cheapest ones)
    int order[GROUP_MAX];
    double cost[GROUP_MAX];
    int64_t tiles[GROUP_MAX];
    for (int i = 0; i < n; ++i) {
        const GemmParams& p = ps[i];
        int bm, bn;
        bm = p.N == 224 ? 128 : 64, bn = p.N;
        tiles[i] = (p.M + bm - 1) / bm * (p.N / bn);
        cost[i] = (double)bm * bn * p.K;
        order[i] = i;
    }
    std::sort(order, order + n, [&](int a, int b) { return cost[a] > cost[b]; });
    GroupedGemmParams g{};
    g.n = n;
    int64_t first = 0;
    for (int k = 0; k < n; ++k) {
        g.p[k] = ps[order[k]];
        g.first[k] = (int)first;
        first += (tiles[order[k]] + 7) / 8 * 8;
        if (first > 0x7fffffff) return fail(PAFUSE_E_ARG, "grouped gemm grid out of range");
    }
    g.first[n] = (int)first;
    for (int k = n + 1; k <= GROUP_MAX; ++k) g.first[k] = (int)first;
    constexpr size_t lds = 2 * DmaTile<2, 2, 6, 16>::STAGE_BYTES;  // the widest variant's ring
    static_assert(lds >= 2 * DmaTile<2, 2, 4, 16>::STAGE_BYTES && lds >= 2 * DmaTile<4, 1, 7, 16>::STAGE_BYTES && lds <= 80 * 1024, "LDS");
    return launch<grouped_rowln_kernel<EPI_ROWLN>>("grouped_rowln_kernel", (unsigned)first, 256, lds, s, g);
}

bool width_supported(int C) { return C == 384 || C == 288 || C == 256 || C == 224 || C == 128 || C == 64; }

// ------------------------------------------------------------------------------------------- attention dispatch
template <int LP, int DP, int NW>
int launch_attn(const AttnParams& p, hipStream_t s) {
    constexpr int ITEMS = NW / (LP / 16);
    constexpr size_t lds = (size_t)2 * ITEMS * LP * (DP + 4) * sizeof(float);
    const int64_t nitems = p.nseq * p.heads;
    const int64_t grid = (nitems + ITEMS - 1) / ITEMS;
    if (grid > 0x7fffffff) return fail(PAFUSE_E_ARG, "attention grid out of range");
    return launch<attn_kernel<LP, DP, NW>>("attn_kernel", (unsigned)grid, NW * 64, lds, s, p);
}

// one item per wave, WPB waves per workgroup; WPB slices of [LP][DP + 4] floats: 12 or more waves per CU in 160 KB of LDS
// (4 x 6.5 KB at <32,48>: six workgroups .. 4 x 11.25 KB at <80,32>: three)
template <int LP, int DP, int WPB>
int launch_attn_wave(const AttnParams& p, hipStream_t s) {
    constexpr size_t lds = (size_t)WPB * LP * (DP + 4) * sizeof(float);
    static_assert(lds <= 64 * 1024 && (160 * 1024 / lds) * WPB >= 12, "LDS");
    const int64_t nitems = p.nseq * p.heads;
    const int64_t grid = (nitems + WPB - 1) / WPB;
    if (grid > 0x7fffffff) return fail(PAFUSE_E_ARG, "attention grid out of range");
    return launch<attn_wave_kernel<LP, DP, WPB>>("attn_wave_kernel", (unsigned)grid, WPB * 64, lds, s, p);
}

template <int DP>
int launch_attn_long(const AttnParams& p, hipStream_t s) {
    constexpr size_t lds = (size_t)2 * ATTN_LONG_LP * (DP + 4) * sizeof(float);   // 104 KB at DP = 48
    static_assert(lds <= 160 * 1024, "LDS");
    const int64_t grid = p.nseq * p.heads;
    if (grid > 0x7fffffff) return fail(PAFUSE_E_ARG, "attention grid out of range");
    return launch<attn_long_kernel<DP>>("attn_long_kernel", (unsigned)grid, 1024, lds, s, p);
}

int attention(const AttnParams& p, hipStream_t s) {
    if (p.nseq <= 0) return PAFUSE_OK;
#ifdef PAFUSE_ABL_NO_ATTENTION   // timing ablation (tools/): what the loop costs with every attention launch removed (results wrong)
    return PAFUSE_OK;
#endif
    if (p.d % 4 || p.d > 48 || p.L > ATTN_LONG_LP || p.L <= 0)
        return fail(PAFUSE_E_SHAPE, "attention: head dim %d (need %%4, <=48) / length %d (need <=%d)", p.d, p.L, ATTN_LONG_LP);
    if (p.L > 144) {   // long temporal sequences (clips of 145 .. 256 frames): fp32 output rows only
        if (p.o_h) return fail(PAFUSE_E_SHAPE, "attention: no f16x2 image output for sequences of %d > 144 tokens: use mode 2", p.L);
        return p.d <= 32 ? launch_attn_long<32>(p, s) : launch_attn_long<48>(p, s);
    }
    const int dp = p.d <= 32 ? 32 : 48;
    const int lp = p.L <= 32 ? 32 : (p.L <= 48 ? 48 : (p.L <= 80 ? 80 : 144));
    if (lp == 144)  // the single-model variant: one sequence of all 134 keypoints (common/diffusionpose.py:150-153)
        return dp == 32 ? launch_attn<144, 32, 9>(p, s) : launch_attn<144, 48, 9>(p, s);
    // one item per wave where that form is the faster one alone (profiles/attention_wave_items.json); the workgroup form keeps
    // <32,32> (the temporal launches of face and hands: 61 against 54 - 58 us, 41 against 38) and <80,48> (161 against 149:
    // its 16 KB slices leave 9 waves a CU)
    if (dp == 32) {
        if (lp == 32) return launch_attn<32, 32, 4>(p, s);
        if (lp == 48) return launch_attn_wave<48, 32, 4>(p, s);
        return launch_attn_wave<80, 32, 4>(p, s);
    }
    if (lp == 32) return launch_attn_wave<32, 48, 4>(p, s);
    if (lp == 48) return launch_attn_wave<48, 48, 4>(p, s);
    return launch_attn<80, 48, 5>(p, s);
}

// --------------------------------------------------------------------------------------- per-part activations
constexpr size_t RANGE_FLAG_BYTES = 256;   // behind pafuse_d3dp_sample's workspace: [0] int32, set when a denoiser output is not finite

struct PartBuffers {
    float *x, *xn, *o, *wide;  // [M,C], [M,C], [M,C], [M,3C] (qkv, then the MLP hidden [M,2C])
    //                            f16x2 mode: xn, o and (as the hidden) wide hold H images of those tensors - same bytes;
    //                            bf16x3 on images (mode 4): X images, 6 bytes per element - xn and o are carved at that size
    //                            (`eb`), the [M,2C] hidden image is exactly the [M,3C] floats of `wide`
    int eb;                    // bytes per element of xn and o: 4, or 6 in mode 4
    float* temb;               // [B,C]
    float* pred;               // [M,3]
    float* stats;              // [M,2] (mean, rstd) of a row when the LayerNorm is folded into the consumer GEMM
};

size_t part_buffer_bytes(int64_t M, int C, int B, int eb = 4) {
    return align_up((size_t)M * C * 4) + 2 * align_up((size_t)M * C * eb) + align_up((size_t)M * 3 * C * 4) + align_up((size_t)B * C * 4) +
           align_up((size_t)M * 3 * 4) + align_up((size_t)M * 2 * 4);
}

char* carve_part(char* base, int64_t M, int C, int B, PartBuffers& pb, int eb = 4) {
    pb.eb = eb;
    pb.x = (float*)base;
    base += align_up((size_t)M * C * 4);
    pb.xn = (float*)base;
    base += align_up((size_t)M * C * eb);
    pb.o = (float*)base;
    base += align_up((size_t)M * C * eb);
    pb.wide = (float*)base;
    base += align_up((size_t)M * 3 * C * 4);
    pb.temb = (float*)base;
    base += align_up((size_t)B * C * 4);
    pb.pred = (float*)base;
    base += align_up((size_t)M * 3 * 4);
    pb.stats = (float*)base;
    base += align_up((size_t)M * 2 * 4);
    return base;
}

// the rows [row0, ...) of a part's buffers (hypotheses are independent, so a part can be cut into hypothesis groups
// that run on different streams; temb and the scratch behind `wide` stay shared / are offset like the rest)
PartBuffers offset_rows(const PartBuffers& pb, int64_t row0, int C) {
    PartBuffers o = pb;
    const int64_t img = row0 * C * pb.eb / 4;   // (floats; C is a multiple of 32)
    o.x = pb.x + row0 * C, o.xn = pb.xn + img, o.o = pb.o + img, o.wide = pb.wide + row0 * 3 * C;
    o.pred = pb.pred + row0 * 3;
    o.stats = pb.stats + row0 * 2;
    return o;
}

static bool ln_folded(const pafuse_mixste2_weights* w) { return w->ste[0].qkv_lt != nullptr; }   // (qkv_ls / fc1_ls: round 3's uncentred form, not read)
// f16x2 with the LayerNorm folded: the residual stream between the blocks lives in memory as its H image only
static bool h_residual_only(const pafuse_mixste2_weights* w) { return mode_images(w->operand_bf16) && ln_folded(w) && !w->keep_f32_residual; }

// The output side of an embed launch, in ONE place (the loop, pafuse_mixste2_forward, pafuse_embed and pafuse_embed_unit): which
// of fp32 rows / normalised rows / image / statistics embed_kernel writes for a product mode, with the first LayerNorm folded
// into the qkv GEMM or not, for the rows [row0, row0 + nrows) of the part's token matrix.  `x`, `xn` and `image` are indexed by
// the ABSOLUTE row; `stats` points at the pair of row row0 (the kernel indexes it by the local row).  In the image pipelines the
// image takes the place of xn (callers that carve one buffer for both pass it twice).
static void embed_outputs(EmbedParams& e, int mode, bool folded, bool h_only, float* x, float* xn, void* image, float* stats,
                          int64_t row0, int64_t nrows) {
    e.x = h_only ? nullptr : x, e.xn = xn;
    e.stats = folded ? stats : nullptr;
    e.xh = mode_images(mode) ? reinterpret_cast<uint8_t*>(image) : nullptr;
    e.x_image = mode == MODE_BF16X3_IMAGES;
    e.centre_x = mode == MODE_BF16X3 && folded;
    e.row0 = row0, e.nrows = nrows;
}

// `training`: the training entry points make the images of the weights they multiply themselves (weights change every step)
int check_weights(const pafuse_mixste2_weights* w, bool training = false) {
    if (!w) return fail(PAFUSE_E_ARG, "null weights");
    static_assert(EMBED_NV * 128 >= 384, "embed kernel covers the widest part");
    if (w->in_chans != 5) return fail(PAFUSE_E_SHAPE, "in_chans must be 5, got %d", w->in_chans);
    if (w->depth < 1 || w->depth > PAFUSE_MAX_DEPTH) return fail(PAFUSE_E_SHAPE, "depth %d out of range", w->depth);
    if (!width_supported(w->channels)) return fail(PAFUSE_E_SHAPE, "channel width %d has no kernel", w->channels);
    if (w->heads <= 0 || w->channels % w->heads) return fail(PAFUSE_E_SHAPE, "heads %d !| C %d", w->heads, w->channels);
    const int d = w->channels / w->heads;
    if (d % 4 || d > 48) return fail(PAFUSE_E_SHAPE, "head dim %d unsupported", d);
    if (w->joints < 1 || w->joints > 144 || w->frames < 1 || w->frames > ATTN_LONG_LP)
        return fail(PAFUSE_E_SHAPE, "sequence lengths J=%d F=%d: J must be in 1..144, F in 1..%d", w->joints, w->frames, ATTN_LONG_LP);
    if (w->operand_bf16 == MODE_F16X2 && w->frames > 144)   // (the long-sequence attention writes fp32 rows, not the f16x2 H image)
        return fail(PAFUSE_E_SHAPE, "f16x2: no attention form for clips of %d > 144 frames: use mode 2", w->frames);
    if (!mode_valid(w->operand_bf16)) return fail(PAFUSE_E_ARG, "matrix-product mode %d", w->operand_bf16);
    if (mode_images(w->operand_bf16)) {   // the image pipelines: the PAFUSE part widths; plain layers that tile by 128 or 224 columns
        const int hidden = w->mlp_hidden > 0 ? w->mlp_hidden : 2 * w->channels;
        if (!hgemm_width(w->channels) || !hgemm_plain_n(3 * w->channels) || !hgemm_plain_n(hidden) || hidden % 32)
            return fail(PAFUSE_E_SHAPE, "the image pipelines (f16x2, bf16x3 on images) serve the widths 224 / 256 / 384 with an MLP hidden "
                                        "width that is a multiple of 128 or 224 (got C = %d, hidden = %d): use mode 2", w->channels, hidden);
    }
    if (w->operand_bf16 == MODE_BF16X3_IMAGES && !training) {   // bf16x3 on images: qkv + attention fused in every block (no unfused attention on X images)
        for (int i = 0; i < w->depth; ++i)
            for (const pafuse_block_weights* b : {&w->ste[i], &w->tte[i]})
                if (!b->qkv_hs || !b->qkv_hb) return fail(PAFUSE_E_ARG, "bf16x3 on images needs the head-major qkv image of every block (qkv_hs, qkv_hb)");
        if (!xfqa_has(w->joints, d, w->heads) || !xfqa_has(w->frames, d, w->heads))
            return fail(PAFUSE_E_SHAPE, "bf16x3 on images: no fused qkv + attention form for sequences of %d / %d tokens at head dim %d, %d heads: "
                                        "use mode 2", w->joints, w->frames, d, w->heads);
    }
    if (w->mlp_hidden < 0 || (w->mlp_hidden > 0 && (w->mlp_hidden % 32 || w->mlp_hidden > 3 * w->channels)))
        return fail(PAFUSE_E_SHAPE, "mlp hidden width %d must be a multiple of 32 and at most 3C = %d", w->mlp_hidden, 3 * w->channels);
    if (!(w->qk_scale >= 0.f)) return fail(PAFUSE_E_ARG, "qk_scale must be positive (0 = head_dim^-0.5)");
    if (training && (w->operand_bf16 == MODE_BF16 || mode_images(w->operand_bf16)))
        return fail(PAFUSE_E_ARG, "training runs fp32 ('f32') or split-precision ('bf16x3') products");
    if (mode_split(w->operand_bf16) && !training)
        for (int i = 0; i < w->depth; ++i)
            for (const pafuse_block_weights* b : {&w->ste[i], &w->tte[i]})
                if ((!b->qkv_ws && w->operand_bf16 != MODE_BF16X3_IMAGES) || !b->proj_ws || !b->fc1_ws || !b->fc2_ws)   // (mode 4 multiplies qkv_hs only)
                    return fail(PAFUSE_E_ARG, "split-precision mode needs the pre-split image of every linear weight "
                                              "(pafuse_split_weights)");
    // a folded LayerNorm (pafuse_block_weights.qkv_lt, fc1_lt) is a property of the whole denoiser: the producer of a block's
    // statistics is the block before it
    const bool fold = ln_folded(w);
    for (int i = 0; i < w->depth; ++i)
        for (const pafuse_block_weights* b : {&w->ste[i], &w->tte[i]}) {
            const int set = (b->qkv_lt != nullptr) + (b->fc1_lt != nullptr);
            if (set != (fold ? 2 : 0)) return fail(PAFUSE_E_ARG, "folded-LayerNorm vectors (qkv_lt, fc1_lt) must be set in every block or in none");
        }
    if (fold && !mode_split(w->operand_bf16)) return fail(PAFUSE_E_ARG, "the folded LayerNorm exists in the split-precision modes only");
    return PAFUSE_OK;
}

// one transformer block on the fixed-layout token matrix; `post`/`next` describe the epilogue of its fc2 GEMM
struct BlockTail {
    const float *post_w, *post_b;
    float post_eps;
    const float* pos;
    int posJ, posF;
    const float *next_w, *next_b;
    float next_eps;
    const float *head_w, *head_b;
    float* out_head;
};

// the five launches of one transformer block, as parameter blocks (run part by part, or grouped across parts)
struct BlockLaunch {
    GemmParams qkv, proj, fc1, fc2;
    AttnParams attn;
    FqaParams fqa;   // qkv + attention in one kernel (fused == true: replaces the qkv and attn launches)
    bool fused;
    MlpParams mlp;   // fc1 -> GELU -> fc2 in one kernel (mlp_fused == true: replaces the fc1 and fc2 launches)
    bool mlp_fused;
};

BlockLaunch make_block(const pafuse_block_weights& bw, const PartBuffers& pb, int64_t M, int C, int heads, int64_t nseq, int L,
                       int64_t group, int64_t group_stride, int64_t seq_stride, int64_t tok_stride, const BlockTail& tail,
                       int mode, int hidden = 0, float qk_scale = 0.f, bool fold = false, bool keep_f32_residual = false) {
    if (hidden <= 0) hidden = 2 * C;  // mlp_ratio = 2, the PAFUSE configuration
    BlockLaunch b{};
    // fold: the LayerNorm in front of qkv / fc1 is applied inside those GEMMs (GemmParams::ln_in); the producer of a row
    // leaves its (mean, rstd) in the part's stats buffer
    float* const stats = pb.stats;
    // f16x2: every GEMM operand is an H image - xn (of x with the fold, else of LN(x)), o, and the MLP hidden in
    // `wide` are written in that form by their producers (hgemm.hpp); the *_ws pointers are the weights' H images
    const bool hp = mode_images(mode);   // (mode 4, bf16x3 on images: the same flow on X images - 6 bytes per element, exact)
    uint8_t* const xn_h = reinterpret_cast<uint8_t*>(pb.xn);
    const bool h_residual = hp && fold && !keep_f32_residual;
    // qkv = LN1(x) Wqkv^T + b        (xn already holds LN1(x))                         mixste.py:65
    GemmParams& g = b.qkv;
    g.A = pb.xn, g.W = bw.qkv_w, g.bias = bw.qkv_b, g.out = pb.wide, g.M = M, g.N = 3 * C, g.K = C, g.act = 0;
    g.mode = mode, g.Wsplit = (const uint8_t*)bw.qkv_ws, g.wlayout = WLAYOUT_M16;   // qkv images are in the M16 layout (include/pafuse_hip.h)
    if (fold) g.A = pb.x, g.ln_in = stats, g.bias = bw.qkv_lt;
    if (hp) g.Ah = xn_h, g.Wh = (const uint8_t*)bw.qkv_ws;
    if (fold) g.ln_s = nullptr;   // x (its image; mode 2: its fp32 rows) is stored centred on the row mean: rstd acc + lt, no mean term
    AttnParams& a = b.attn;
    a.qkv = pb.wide, a.o = pb.o, a.nseq = nseq, a.L = L, a.C = C, a.heads = heads, a.d = C / heads;
    a.group = group, a.group_stride = group_stride, a.seq_stride = seq_stride, a.tok_stride = tok_stride;
    a.scale = qk_scale != 0.f ? qk_scale : 1.0f / sqrtf((float)(C / heads));  // qk_scale or head_dim ** -0.5  mixste.py:52
    if (hp) a.o_h = reinterpret_cast<uint8_t*>(pb.o);
    // the two in one kernel where a head-major image was supplied and the shape has a fused form
    b.fused = false;
    if (mode_split(mode) && bw.qkv_hs && bw.qkv_hb && (mode == MODE_BF16X3_IMAGES ? xfqa_has(L, C / heads, heads) : fqa_has(L, C / heads, mode))) {   // (qkv_hl, round 3's uncentred term, is not read: not required)
        const int lp = fqa_lp(L, mode), dp = fqa_dp(C / heads);
        FqaParams& f = b.fqa;
        f.g = g;
        f.g.Wsplit = (const uint8_t*)bw.qkv_hs, f.g.bias = bw.qkv_hb, f.g.ln_s = nullptr;
        if (hp) f.g.Wh = (const uint8_t*)bw.qkv_hs, f.g.ln_s = nullptr;   // (Ah is the qkv launch's: centred; o is written as an H image)
        f.g.N = heads * 3 * dp;
        f.o = pb.o, f.nseq = nseq, f.L = L, f.C = C, f.heads = heads, f.d = C / heads;
        f.nseq_tile = fqa_nseq_tile(L, lp);   // whole sequences per tile, the last one's LP-row key tile inside the buffer
        f.group = group, f.group_stride = group_stride, f.seq_stride = seq_stride, f.tok_stride = tok_stride;
        f.scale = a.scale;
        b.fused = f.nseq_tile * L <= fqa_tile_rows(lp);
    }
    // x = x + o Wproj^T + b ; xn = LN2(x)                                               mixste.py:80,114-115
    GemmParams& pj = b.proj;
    pj.A = pb.o, pj.W = bw.proj_w, pj.bias = bw.proj_b, pj.M = M, pj.N = C, pj.K = C;
    pj.resid = pb.x, pj.out_x = pb.x, pj.out_n = pb.xn;
    pj.next_w = bw.norm2_w, pj.next_b = bw.norm2_b, pj.next_eps = 1e-6f;
    pj.mode = mode, pj.Wsplit = (const uint8_t*)bw.proj_ws;
    if (fold) pj.out_n = nullptr, pj.ln_stats = stats;
    if (hp) {
        pj.Ah = reinterpret_cast<const uint8_t*>(pb.o), pj.Wh = (const uint8_t*)bw.proj_ws;
        // folded: the residual stream lives in memory as the H image of x ONLY - read as the residual, written back in place
        // (a workgroup owns its rows), and it IS the next GEMM's operand; no fp32 x is read or written inside the denoiser
        if (fold && h_residual) pj.out_xh = xn_h, pj.resid_h = xn_h, pj.resid = nullptr, pj.out_x = nullptr;
        else if (fold) pj.out_xh = xn_h;
        else pj.out_n = nullptr, pj.out_nh = xn_h;
    }
    // h = GELU(xn W1^T + b1)                                                            mixste.py:38-39
    GemmParams& f1 = b.fc1;
    f1.A = pb.xn, f1.W = bw.fc1_w, f1.bias = bw.fc1_b, f1.out = pb.wide, f1.M = M, f1.N = hidden, f1.K = C, f1.act = 1;
    f1.mode = mode, f1.Wsplit = (const uint8_t*)bw.fc1_ws, f1.wlayout = WLAYOUT_M16;   // (round 6: fc1 images are in the M16 layout too)
    if (fold) f1.A = pb.x, f1.ln_in = stats, f1.bias = bw.fc1_lt;
    if (hp) f1.Ah = xn_h, f1.Wh = (const uint8_t*)bw.fc1_ws, f1.out_h = reinterpret_cast<uint8_t*>(pb.wide);
    if (fold) f1.ln_s = nullptr;
    // x = post(x + h W2^T + b2) [+ pos] ; xn = next(x) | head                           mixste.py:41,115,243,250,257
    GemmParams& f2 = b.fc2;
    f2.A = pb.wide, f2.W = bw.fc2_w, f2.bias = bw.fc2_b, f2.M = M, f2.N = C, f2.K = hidden;
    f2.resid = pb.x, f2.out_x = tail.out_head ? nullptr : pb.x, f2.out_n = tail.out_head ? nullptr : pb.xn;
    f2.post_w = tail.post_w, f2.post_b = tail.post_b, f2.post_eps = tail.post_eps;
    f2.pos = tail.pos, f2.posJ = tail.posJ, f2.posF = tail.posF;
    f2.next_w = tail.next_w, f2.next_b = tail.next_b, f2.next_eps = tail.next_eps;
    f2.head_w = tail.head_w, f2.head_b = tail.head_b, f2.out_head = tail.out_head;
    if (!tail.next_w) f2.out_n = nullptr;
    if (fold && tail.next_w && !tail.out_head) f2.out_n = nullptr, f2.ln_stats = stats;   // the head keeps its own LayerNorm
    f2.mode = mode, f2.Wsplit = (const uint8_t*)bw.fc2_ws;
    if (hp) {
        f2.Ah = reinterpret_cast<const uint8_t*>(pb.wide), f2.Wh = (const uint8_t*)bw.fc2_ws;
        if (f2.ln_stats) f2.out_xh = xn_h;                       // folded: the next block's qkv reads the H image of x
        else if (f2.out_n) f2.out_n = nullptr, f2.out_nh = xn_h;  // not folded: the H image of the next LayerNorm's output
        if (fold && h_residual) {
            f2.resid_h = xn_h, f2.resid = nullptr;
            if (f2.out_xh) f2.out_x = nullptr;                    // (the head's block writes neither)
        }
    }
    // the two MLP launches as one kernel: the hidden activations stay in registers (hgemm.hpp hmlp_kernel); fc2_hp is the H
    // image of fc2.weight with the columns of each group of 16 in the order the kernel's accumulators hand them over
    b.mlp_fused = false;
    if (h_residual && mode == MODE_F16X2 && bw.fc2_hp && hmlp_has(C, hidden)) {
        MlpParams& m = b.mlp;
        m.g = f2;
        m.g.Ah = xn_h, m.g.Wh = (const uint8_t*)bw.fc2_hp;
        m.W1h = (const uint8_t*)bw.fc1_ws, m.bias1 = f1.bias, m.ln_in = f1.ln_in;
        b.mlp_fused = true;
    }
    return b;
}

// ---- PAFUSE_DIAG builds only: a hash of every intermediate tensor of a denoiser pass, written by a tiny kernel queued right
// behind its producer (tests/cabi/queue_concurrency.c compares the hashes of a concurrent run with the single-stream ones:
// the FIRST slot that differs names the kernel that went wrong on right inputs)
#ifdef PAFUSE_DIAG
thread_local unsigned long long* g_trace = nullptr;   // device array of slots, zeroed by the caller
thread_local int g_trace_n = 0, g_trace_i = 0;
thread_local float* g_snap = nullptr;                 // device buffer [M*C (+ B*C)]: copy of x right behind embed_kernel,
//                                                       then of temb taken between time_embed_kernel and embed_kernel
__global__ void trace_hash_kernel(const uint32_t* data, int64_t words, unsigned long long* slot) {
    unsigned long long h = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256)
        h += (unsigned long long)data[i] * (2 * (unsigned long long)i + 1);      // order-independent sum
    for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(slot, h);
}
void trace(const void* buf, size_t bytes, hipStream_t s) {
    if (!g_trace || g_trace_i >= g_trace_n) return;
    hipLaunchKernelGGL(trace_hash_kernel, dim3(64), dim3(256), 0, s, (const uint32_t*)buf, (int64_t)(bytes / 4), g_trace + g_trace_i++);
}
#define PAFUSE_TRACE(buf, bytes, s) trace(buf, bytes, s)
#else
#define PAFUSE_TRACE(buf, bytes, s)
#endif

// one block of n independent parts: the same layer of every part in one grid where the grouped kernels apply
// (n == 1: the plain per-part launches)
int run_blocks(const BlockLaunch* bl, int n, hipStream_t s, bool gemms_only = false, double* flops = nullptr,
               int* launches = nullptr, int layer_mask = 15, bool shared_grids = true) {
    int rc;
    GemmParams g[GROUP_MAX];
    auto count = [&](int layers) {
        if (!flops) return;
        for (int i = 0; i < n; ++i) *flops += 2.0 * g[i].M * g[i].N * g[i].K;
        *launches += layers;
    };
    auto layer_of = [&](const BlockLaunch* bl, int n, GemmParams BlockLaunch::*which, bool rowln, int bit) -> int {
        if (!(layer_mask & bit)) return PAFUSE_OK;
        const bool grouped = shared_grids && n >= 2;
        bool all = grouped;
        for (int i = 0; i < n; ++i) {
            g[i] = bl[i].*which;
            all = all && rowln && g[i].M > 0 && group_ok_rowln(g[i]);
        }
        const int r = rowln ? gemm_group<true>(g, n, s, shared_grids) : gemm_group<false>(g, n, s, shared_grids);
        if (flops) {
            for (int i = 0; i < n; ++i) *flops += 2.0 * g[i].M * g[i].N * g[i].K;
            *launches += all ? 1 : n;
        }
        for (int i = 0; i < n; ++i) {
            if (rowln) {
                if (g[i].out_x) PAFUSE_TRACE(g[i].out_x, (size_t)g[i].M * g[i].N * 4, s);
                if (g[i].out_n) PAFUSE_TRACE(g[i].out_n, (size_t)g[i].M * g[i].N * 4, s);
            } else {
                PAFUSE_TRACE(g[i].out, (size_t)g[i].M * g[i].N * 4, s);
            }
        }
        return r;
    };
    // qkv -> attention stays part by part: a part's qkv rows (119 - 197 MB at P = 20) are read back by its attention
    // while they are still in the 256 MB Infinity Cache; written for all parts first (455 MB) they are not, and the six
    // attention launches of a block pair get 21 us slower, more than the shared qkv grid saves (9 us; rocprofv3, r02)
    for (int i = 0; i < n; ++i) {
        g[i] = bl[i].qkv;
        if (bl[i].fused) {   // one kernel: the GEMM replay (gemms_only) cannot leave its attention phase out
            if ((layer_mask & 1) && (rc = fused_qkv_attention(bl[i].fqa, s))) return rc;
            PAFUSE_TRACE(bl[i].attn.o, (size_t)g[i].M * bl[i].attn.C * 4, s);
            continue;
        }
        if (g[i].mode == MODE_BF16X3_IMAGES) return fail(PAFUSE_E_SHAPE, "bf16x3 on images: this block has no fused qkv + attention form");
        if ((layer_mask & 1) && (rc = gemm_bias(g[i], s))) return rc;
        PAFUSE_TRACE(g[i].out, (size_t)g[i].M * g[i].N * 4, s);
        if (!gemms_only && (rc = attention(bl[i].attn, s))) return rc;
        PAFUSE_TRACE(bl[i].attn.o, (size_t)g[i].M * bl[i].attn.C * 4, s);
    }
    if (layer_mask & 1) count(n);
    if ((rc = layer_of(bl, n, &BlockLaunch::proj, true, 2))) return rc;
    // the MLP: one kernel where the part's block has the fused form (a replay of the fc1 layer alone runs it, of fc2 alone
    // nothing of that part), the fc1 and fc2 launches for the other parts
    BlockLaunch rest[GROUP_MAX];
    int nrest = 0;
    for (int i = 0; i < n; ++i) {
        if (!bl[i].mlp_fused) {
            rest[nrest++] = bl[i];
            continue;
        }
        if (!(layer_mask & 4)) continue;
        if ((rc = fused_mlp(bl[i].mlp, s))) return rc;
        if (flops) *flops += 2.0 * (2.0 * bl[i].fc1.M * bl[i].fc1.N * bl[i].fc1.K), *launches += 1;
        if (bl[i].mlp.g.out_xh) PAFUSE_TRACE(bl[i].mlp.g.out_xh, (size_t)bl[i].fc2.M * bl[i].fc2.N * 4, s);
    }
    if (!nrest) return PAFUSE_OK;
    if ((rc = layer_of(rest, nrest, &BlockLaunch::fc1, false, 4))) return rc;
    return layer_of(rest, nrest, &BlockLaunch::fc2, true, 8);
}

int run_block(const pafuse_block_weights& bw, const PartBuffers& pb, int64_t M, int C, int heads, int64_t nseq, int L,
              int64_t group, int64_t group_stride, int64_t seq_stride, int64_t tok_stride, const BlockTail& tail,
              hipStream_t s, bool gemms_only = false, double* flops = nullptr, int* launches = nullptr, int mode = MODE_F32) {
    const BlockLaunch b = make_block(bw, pb, M, C, heads, nseq, L, group, group_stride, seq_stride, tok_stride, tail, mode);
    return run_blocks(&b, 1, s, gemms_only, flops, launches);
}

// the 2*depth blocks + head of n independent MixSTE2 denoisers of equal depth on rows already embedded in pb[i].x /
// pb[i].xn; results in pb[i].pred [M_i,3].  Block k of every part is issued together (run_blocks).
int run_mixste_layers_n(const pafuse_mixste2_weights* const* ws, const PartBuffers* pbs, const int64_t* Rs, int n,
                        hipStream_t s, bool gemms_only = false, double* flops = nullptr, int* launches = nullptr,
                        int layer_mask = 15, bool shared_grids = true) {
    if (n < 1 || n > GROUP_MAX) return fail(PAFUSE_E_ARG, "run_mixste_layers_n: %d parts", n);
    for (int i = 1; i < n; ++i)
        if (ws[i]->depth != ws[0]->depth) return fail(PAFUSE_E_ARG, "run_mixste_layers_n: parts of unequal depth");
    int rc;
    BlockLaunch bl[GROUP_MAX];
    for (int i = 0; i < ws[0]->depth; ++i) {
        for (int k = 0; k < n; ++k) {
            const pafuse_mixste2_weights* w = ws[k];
            const int F = w->frames, J = w->joints, C = w->channels;
            BlockTail t{};
            // spatial block i: sequences = the J joints of one (r, f); then Spatial_norm; TTE block 0 first adds the
            // temporal position embedding; the next LayerNorm is norm1 of temporal block i.
            t.post_w = w->snorm_w, t.post_b = w->snorm_b, t.post_eps = 1e-6f;
            if (i == 0) t.pos = w->pos_temporal, t.posJ = J, t.posF = F;
            t.next_w = w->tte[i].norm1_w, t.next_b = w->tte[i].norm1_b, t.next_eps = 1e-6f;
            bl[k] = make_block(w->ste[i], pbs[k], Rs[k] * F * J, C, w->heads, Rs[k] * F, J, 1, J, 0, 1, t, w->operand_bf16,
                               w->mlp_hidden, w->qk_scale, ln_folded(w), w->keep_f32_residual != 0);
        }
        if ((rc = run_blocks(bl, n, s, gemms_only, flops, launches, layer_mask, shared_grids))) return rc;
        for (int k = 0; k < n; ++k) {
            const pafuse_mixste2_weights* w = ws[k];
            const int F = w->frames, J = w->joints, C = w->channels;
            // temporal block i: sequences = the F frames of one (r, j); then Temporal_norm; next is norm1 of spatial
            // block i+1, or the head (LayerNorm eps 1e-5 + Linear(C,3)) after the last block.
            BlockTail t{};
            t.post_w = w->tnorm_w, t.post_b = w->tnorm_b, t.post_eps = 1e-6f;
            if (i + 1 < w->depth) {
                t.next_w = w->ste[i + 1].norm1_w, t.next_b = w->ste[i + 1].norm1_b, t.next_eps = 1e-6f;
            } else {
                t.next_w = w->hnorm_w, t.next_b = w->hnorm_b, t.next_eps = 1e-5f;
                t.head_w = w->head_w, t.head_b = w->head_b, t.out_head = pbs[k].pred;
            }
            bl[k] = make_block(w->tte[i], pbs[k], Rs[k] * F * J, C, w->heads, Rs[k] * J, F, J, (int64_t)F * J, 1, J, t,
                               w->operand_bf16, w->mlp_hidden, w->qk_scale, ln_folded(w), w->keep_f32_residual != 0);
        }
        if ((rc = run_blocks(bl, n, s, gemms_only, flops, launches, layer_mask, shared_grids))) return rc;
    }
    return PAFUSE_OK;
}

int run_mixste_layers(const pafuse_mixste2_weights* w, const PartBuffers& pb, int64_t R, hipStream_t s,
                      bool gemms_only = false, double* flops = nullptr, int* launches = nullptr, int layer_mask = 15) {
    return run_mixste_layers_n(&w, &pb, &R, 1, s, gemms_only, flops, launches, layer_mask);
}

// parts of one configuration may share grids when they all run split-precision products and have the same depth
bool parts_groupable(const pafuse_d3dp_config* cfg) {
    if (cfg->part_by_part_launches || cfg->num_parts < 2 || cfg->num_parts > GROUP_MAX) return false;
    for (int i = 0; i < cfg->num_parts; ++i)
        if (cfg->part[i].operand_bf16 != MODE_BF16X3 || cfg->part[i].depth != cfg->part[0].depth) return false;
    return true;
}

int launch_time_embed(const pafuse_mixste2_weights* w, const int64_t* t, int64_t t_scalar, int B, float* out,
                      float* hid_scratch, hipStream_t s) {
    TimeEmbedParams p{};
    const int C = w->channels;
    p.t = t, p.t_scalar = t_scalar, p.freqs = w->freqs;
    p.w1 = w->tm1_w, p.b1 = w->tm1_b, p.w3 = w->tm3_w, p.b3 = w->tm3_b, p.hid = hid_scratch, p.out = out, p.C = C;
    if (int rc = launch<time_embed_kernel<0>>("time_embed_kernel", dim3((2 * C + 7) / 8, B), 512, (size_t)C * sizeof(float), s, p)) return rc;
    return launch<time_embed_kernel<1>>("time_embed_kernel", dim3((C + 7) / 8, B), 512, (size_t)2 * C * sizeof(float), s, p);
}

__global__ void copy_kernel(const float* src, float* dst, int64_t n) {
    PAFUSE_XQ_GUARD();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

#include "train_host.inc"

}  // namespace

// ================================================================================================== C ABI
extern "C" {

const char* pafuse_version(void) {
#ifdef PAFUSE_NO_PACKED_F32
    return "pafuse_hip 0.5 (gfx950, f32 MFMA + split bf16x3 / f16x2 MFMA, no packed-fp32 VALU)";
#else
    return "pafuse_hip 0.5 (gfx950, f32 MFMA + split bf16x3 / f16x2 MFMA, packed-fp32 VALU: 16-bit MFMA modes on one stream)";
#endif
}
const char* pafuse_last_error(void) { return g_err; }
int pafuse_abi_version(void) { return PAFUSE_ABI_VERSION; }

#ifdef PAFUSE_DIAG
/* diagnostic builds only (not declared in include/pafuse_hip.h): hash every intermediate of the following passes of this
 * thread into slots[0 .. n) (device memory, zeroed by the caller); returns how many slots the previous passes used */
int pafuse_diag_trace(unsigned long long* slots, int32_t n) {
    const int used = g_trace_i;
    g_trace = slots, g_trace_n = n, g_trace_i = 0;
    return used;
}
void pafuse_diag_snapshot(float* x_copy) { g_snap = x_copy; }
#endif

int pafuse_linear(const float* A, const float* W, const float* bias, float* out, int64_t M, int32_t N, int32_t K,
                  int32_t act, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!A || !W || !bias || !out || M < 0) return fail(PAFUSE_E_ARG, "linear: null pointer or negative M");
    GemmParams g{};
    g.A = A, g.W = W, g.bias = bias, g.out = out, g.M = M, g.N = N, g.K = K, g.act = act & 1, g.mode = (act >> 1) & 1;
    return gemm_bias(g, (hipStream_t)stream);
}

size_t pafuse_split_weights_bytes(int64_t N, int64_t K) { return (N > 0 && K > 0) ? wsplit_bytes(N, K) : 0; }
size_t pafuse_split_image_bytes(int64_t N, int64_t K, int32_t layout) {
    if (N <= 0 || K <= 0) return 0;
    return (layout & PAFUSE_SPLIT_F16X2) && !(layout & PAFUSE_SPLIT_X) ? hsplit_bytes(N, K) : wsplit_bytes(N, K);
}

int pafuse_mode_supported(int32_t mode, int32_t C, int32_t hidden, int32_t heads, int32_t joints, int32_t frames) {
    if (!mode_valid(mode) || heads <= 0 || C <= 0 || C % heads) return 0;
    if (hidden <= 0) hidden = 2 * C;
    const int d = C / heads;
    if (!width_supported(C) || d % 4 || d > 48 || joints < 1 || joints > 144 || frames < 1 || frames > ATTN_LONG_LP) return 0;
    if (mode == MODE_F16X2 && frames > 144) return 0;
    if (mode_images(mode) && (!hgemm_width(C) || !hgemm_plain_n(3 * C) || !hgemm_plain_n(hidden) || hidden % 32)) return 0;
    if (mode == MODE_BF16X3_IMAGES && (!xfqa_has(joints, d, heads) || !xfqa_has(frames, d, heads))) return 0;
    return 1;
}

int pafuse_mixste2_fused_blocks(const pafuse_mixste2_weights* w) {
    int rc = check_weights(w);
    if (rc) return rc;
    const int d = w->channels / w->heads;
    const bool fold = ln_folded(w);
    int n = 0;
    for (int i = 0; i < w->depth; ++i) {
        const pafuse_block_weights* pair[2] = {&w->ste[i], &w->tte[i]};
        const int len[2] = {w->joints, w->frames};
        for (int k = 0; k < 2; ++k)   // the condition of make_block, plus the tile-capacity check it makes
            if (mode_split(w->operand_bf16) && pair[k]->qkv_hs && pair[k]->qkv_hb &&
                (w->operand_bf16 == MODE_BF16X3_IMAGES ? xfqa_has(len[k], d, w->heads) : fqa_has(len[k], d, w->operand_bf16)) &&
                true) {   // (no qkv_hl requirement: nothing reads it since the centred fold of round 5)
                const int lp = fqa_lp(len[k], w->operand_bf16);
                n += (fqa_nseq_tile(len[k], lp) * len[k] <= fqa_tile_rows(lp)) ? 1 : 0;
            }
    }
    return n;
}

int pafuse_split_weights(const float* W, int32_t N, int32_t K, int32_t layout, void* out, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!W || !out) return fail(PAFUSE_E_ARG, "split_weights: null pointer");
    if (N <= 0 || K <= 0 || K % BK) return fail(PAFUSE_E_SHAPE, "split_weights: N=%d, K=%d (K must be a positive multiple of 32)", N, K);
    const int64_t n = (int64_t)N * (K / 8);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (layout & PAFUSE_SPLIT_X) {   // the X image (bf16x3 on the LDS-DMA pipeline): one geometry for every layer, no scaling, no tail
        return launch<xsplit_weights_kernel>("xsplit_weights_kernel", grid, 256, 0, (hipStream_t)stream, W, (uint8_t*)out, N, K);
    }
    if (layout & PAFUSE_SPLIT_F16X2) {   // the f16x2 H image (one geometry for every layer): largest |W| first, then the slices
        hipStream_t st = (hipStream_t)stream;
        uint8_t* const tail = (uint8_t*)out + (size_t)N * K * 4;
        if (hipMemsetAsync(tail, 0, HSPLIT_TAIL_BYTES, st) != hipSuccess) return fail(PAFUSE_E_HIP, "split_weights: memset failed");
        const int64_t elems = (int64_t)N * K;
        if (int rc = launch<absmax_kernel>("hsplit_weights_kernel", (unsigned)std::min<int64_t>((elems + 255) / 256, 1024), 256, 0, st, W, elems,
                                           reinterpret_cast<uint32_t*>(tail) + 1))
            return rc;
        return launch<hsplit_weights_kernel>("hsplit_weights_kernel", grid, 256, 0, st, W, (uint8_t*)out, N, K);
    }
    if (layout < WLAYOUT_PLAIN || layout > WLAYOUT_M16) return fail(PAFUSE_E_ARG, "split_weights: layout %d (0 plain, 1 whole-row, 2 qkv; or PAFUSE_SPLIT_F16X2)", layout);
#ifdef PAFUSE_QKV_32X32
    if (layout == WLAYOUT_M16) layout = WLAYOUT_PLAIN;
#endif
    if (layout == WLAYOUT_M16)
        return launch<split_weights_kernel<32, 1>>("split_weights_kernel", grid, 256, 0, (hipStream_t)stream, W, (uint8_t*)out, N, K);
    if (wsplit_chunk(N, layout == WLAYOUT_ROWLN) == 16)
        return launch<split_weights_kernel<16>>("split_weights_kernel", grid, 256, 0, (hipStream_t)stream, W, (uint8_t*)out, N, K);
    return launch<split_weights_kernel<32>>("split_weights_kernel", grid, 256, 0, (hipStream_t)stream, W, (uint8_t*)out, N, K);
}

int pafuse_linear_split(const float* A, const void* Wsplit, const float* bias, float* out, int64_t M, int32_t N, int32_t K,
                        int32_t act, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!A || !Wsplit || !bias || !out || M < 0) return fail(PAFUSE_E_ARG, "linear_split: null pointer or negative M");
    GemmParams g{};
    g.A = A, g.Wsplit = (const uint8_t*)Wsplit, g.bias = bias, g.out = out, g.M = M, g.N = N, g.K = K, g.act = act & 1;
    g.mode = MODE_BF16X3, g.wlayout = (act & 2) ? WLAYOUT_M16 : WLAYOUT_PLAIN;
    return gemm_bias(g, (hipStream_t)stream);
}

// the whole-row unit entries: check one argument set and turn it into the GemmParams run_blocks / the training forward build
static int rowln_params(const pafuse_rowln_args* a, GemmParams& g) {
    if (!a) return fail(PAFUSE_E_ARG, "linear_rowln: null arguments");
    const int mode = a->operand_bf16;
    if (!mode_valid(mode)) return fail(PAFUSE_E_ARG, "linear_rowln: matrix-product mode %d", mode);
    if (a->M < 0) return fail(PAFUSE_E_ARG, "linear_rowln: negative M");
    if (a->training && mode != MODE_F32 && mode != MODE_BF16X3) return fail(PAFUSE_E_ARG, "linear_rowln: training runs modes 0 and 2 only, got %d", mode);
    const bool img = mode_images(mode);
    if (img ? !hgemm_width(a->N) : !width_supported(a->N))
        return fail(PAFUSE_E_SHAPE, "linear_rowln: no whole-row kernel for width %d in mode %d", a->N, mode);
    if (a->K <= 0 || a->K % BK) return fail(PAFUSE_E_SHAPE, "linear_rowln: K=%d must be a positive multiple of 32", a->K);
    if (!a->bias) return fail(PAFUSE_E_ARG, "linear_rowln: no bias");
    if (img) {
        if (!a->A_img || !a->Wsplit) return fail(PAFUSE_E_ARG, "linear_rowln: mode %d needs the images of A and W (A_img, Wsplit)", mode);
        if (!a->resid == !a->resid_img) return fail(PAFUSE_E_ARG, "linear_rowln: mode %d takes exactly one residual (resid or resid_img)", mode);
    } else {
        if (!a->A || !a->resid) return fail(PAFUSE_E_ARG, "linear_rowln: no A or no residual");
        if (a->A_img || a->resid_img || a->out_x_img || a->out_n_img) return fail(PAFUSE_E_ARG, "linear_rowln: images exist in modes 3 and 4 only");
        if (mode == MODE_BF16X3 && !a->Wsplit) return fail(PAFUSE_E_ARG, "linear_rowln: mode 2 needs the layout-1 image of W (Wsplit)");
        if ((mode != MODE_BF16X3 || a->training) && !a->W) return fail(PAFUSE_E_ARG, "linear_rowln: no fp32 weight W");
    }
    if (!a->post_w != !a->post_b) return fail(PAFUSE_E_ARG, "linear_rowln: post_w and post_b go together");
    if (!a->next_w != !a->next_b) return fail(PAFUSE_E_ARG, "linear_rowln: next_w and next_b go together");
    const bool head = a->head_w || a->head_b || a->out_head;
    if (head && !(a->head_w && a->head_b && a->out_head)) return fail(PAFUSE_E_ARG, "linear_rowln: head needs head_w, head_b and out_head");
    if (head && !a->next_w) return fail(PAFUSE_E_ARG, "linear_rowln: head without next LayerNorm");
    if (a->ln_stats && !a->next_w) return fail(PAFUSE_E_ARG, "linear_rowln: ln_stats without next LayerNorm");
    if (a->ln_stats && head) return fail(PAFUSE_E_ARG, "linear_rowln: ln_stats together with the head");
    if ((a->out_n || a->out_n_img) && (!a->next_w || a->ln_stats)) return fail(PAFUSE_E_ARG, "linear_rowln: out_n needs next LayerNorm without ln_stats");
    if (a->pos && (a->posJ <= 0 || a->posF <= 0)) return fail(PAFUSE_E_ARG, "linear_rowln: pos with posJ=%d, posF=%d", a->posJ, a->posF);
    if (!a->training && (a->rowscale || a->out_pre)) return fail(PAFUSE_E_ARG, "linear_rowln: rowscale / out_pre without training");
    if (a->rowscale && (a->rs_J <= 0 || (a->rs_temporal && a->rs_FJ <= 0)))
        return fail(PAFUSE_E_ARG, "linear_rowln: rowscale with rs_J=%d, rs_FJ=%d", a->rs_J, a->rs_FJ);
    g = GemmParams{};
    g.A = a->A, g.W = a->W, g.bias = a->bias, g.M = a->M, g.N = a->N, g.K = a->K, g.mode = mode;
    g.Wsplit = mode == MODE_BF16X3 ? (const uint8_t*)a->Wsplit : nullptr;
    g.resid = a->resid, g.out_x = a->out_x, g.out_n = a->out_n;
    g.post_w = a->post_w, g.post_b = a->post_b, g.post_eps = a->post_eps;
    g.pos = a->pos, g.posJ = a->posJ, g.posF = a->posF;
    g.next_w = a->next_w, g.next_b = a->next_b, g.next_eps = a->next_eps;
    g.head_w = a->head_w, g.head_b = a->head_b, g.out_head = a->out_head;
    g.ln_stats = a->ln_stats;
    if (img) {
        g.Ah = (const uint8_t*)a->A_img, g.Wh = (const uint8_t*)a->Wsplit;
        g.resid_h = (const uint8_t*)a->resid_img;
        g.out_xh = (uint8_t*)a->out_x_img, g.out_nh = (uint8_t*)a->out_n_img;
    }
    g.rowscale = a->rowscale, g.rs_temporal = a->rs_temporal, g.rs_J = a->rs_J, g.rs_FJ = a->rs_FJ, g.out_pre = a->out_pre;
    return PAFUSE_OK;
}

int pafuse_linear_rowln(const pafuse_rowln_args* a, void* stream) {
    StreamDevice on_stream_device(stream);
    GemmParams g;
    const int rc = rowln_params(a, g);
    if (rc) return rc;
    if (g.M == 0) return PAFUSE_OK;
    return a->training ? gemm_rowln_train(g, (hipStream_t)stream) : gemm_rowln(g, (hipStream_t)stream);
}

int pafuse_linear_rowln_group(const pafuse_rowln_args* a, int32_t n, int32_t shared_grid, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!a || n < 1 || n > GROUP_MAX) return fail(PAFUSE_E_ARG, "linear_rowln_group: %d layers (1 .. %d)", n, GROUP_MAX);
    GemmParams g[GROUP_MAX];
    int live = 0;
    for (int i = 0; i < n; ++i) {
        const int rc = rowln_params(&a[i], g[live]);
        if (rc) return rc;
        if (a[i].training) return fail(PAFUSE_E_ARG, "linear_rowln_group: training layers run one by one (pafuse_linear_rowln)");
        if (g[live].M > 0) ++live;   // (an empty layer launches nothing, as in pafuse_linear_rowln)
    }
    if (!live) return PAFUSE_OK;
    return gemm_group<true>(g, live, (hipStream_t)stream, shared_grid != 0);
}

int pafuse_hsplit_rows(const float* X, int64_t R, int32_t K, void* out, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!X || !out || R < 0) return fail(PAFUSE_E_ARG, "hsplit_rows: null pointer or negative row count");
    if (K <= 0 || K % 8) return fail(PAFUSE_E_SHAPE, "hsplit_rows: K=%d must be a positive multiple of 8", K);
    if (R == 0) return PAFUSE_OK;
    const int64_t n = R * (K / 8);
    if ((n + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "hsplit_rows: grid out of range");
    return launch<hsplit_rows_kernel>("hsplit_rows_kernel", blocks_for(n), 256, 0, (hipStream_t)stream, X, (uint8_t*)out, R, K);
}

int pafuse_xsplit_rows(const float* X, int64_t R, int32_t K, void* out, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!X || !out || R < 0) return fail(PAFUSE_E_ARG, "xsplit_rows: null pointer or negative row count");
    if (K <= 0 || K % 32) return fail(PAFUSE_E_SHAPE, "xsplit_rows: K=%d must be a positive multiple of 32", K);
    if (R == 0) return PAFUSE_OK;
    const int64_t n = R * (K / 8);
    if ((n + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "xsplit_rows: grid out of range");
    return launch<xsplit_rows_kernel>("xsplit_rows_kernel", blocks_for(n), 256, 0, (hipStream_t)stream, X, (uint8_t*)out, R, K);
}

int pafuse_linear_x(const void* Ax, const void* Wx, const float* bias, float* out, void* out_x, int64_t M, int32_t N, int32_t K,
                    int32_t act, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!Ax || !Wx || !bias || (!out && !out_x) || M < 0) return fail(PAFUSE_E_ARG, "linear_x: null pointer or negative M");
    GemmParams g{};
    g.Ah = (const uint8_t*)Ax, g.Wh = (const uint8_t*)Wx, g.bias = bias, g.out = out, g.out_h = (uint8_t*)out_x;
    g.M = M, g.N = N, g.K = K, g.act = act & 1, g.mode = MODE_BF16X3_IMAGES;
    return gemm_bias(g, (hipStream_t)stream);
}

int pafuse_linear_h(const void* Ah, const void* Wh, const float* bias, float* out, void* out_h, int64_t M, int32_t N, int32_t K,
                    int32_t act, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!Ah || !Wh || !bias || (!out && !out_h) || M < 0) return fail(PAFUSE_E_ARG, "linear_h: null pointer or negative M");
    GemmParams g{};
    g.Ah = (const uint8_t*)Ah, g.Wh = (const uint8_t*)Wh, g.bias = bias, g.out = out, g.out_h = (uint8_t*)out_h;
    g.M = M, g.N = N, g.K = K, g.act = act & 1, g.mode = MODE_F16X2;
    return gemm_bias(g, (hipStream_t)stream);
}

int pafuse_qkv_attention_image(int32_t scheme, const void* x_img, const float* stats, const void* qkv_hs, const float* qkv_hb, void* o_img,
                               int64_t M, int64_t nseq, int32_t L, int32_t C, int32_t heads, int64_t group, int64_t group_stride,
                               int64_t seq_stride, int64_t tok_stride, float qk_scale, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!x_img || !qkv_hs || !qkv_hb || !o_img || M < 0 || nseq < 0 || group <= 0) return fail(PAFUSE_E_ARG, "qkv_attention_image: bad argument");
    if (scheme != PAFUSE_SPLIT_F16X2 && scheme != PAFUSE_SPLIT_X) return fail(PAFUSE_E_ARG, "qkv_attention_image: scheme must be PAFUSE_SPLIT_F16X2 or PAFUSE_SPLIT_X");
    if (heads <= 0 || C <= 0 || C % heads || C % 32) return fail(PAFUSE_E_SHAPE, "qkv_attention_image: C=%d, heads=%d", C, heads);
    const int mode = scheme == PAFUSE_SPLIT_X ? MODE_BF16X3_IMAGES : MODE_F16X2, d = C / heads;
    if (L <= 0 || !(mode == MODE_BF16X3_IMAGES ? xfqa_has(L, d, heads) : fqa_has(L, d, MODE_F16X2)))
        return fail(PAFUSE_E_SHAPE, "qkv_attention_image: no fused form for sequences of %d tokens at head dim %d", L, d);
    if (nseq == 0) return PAFUSE_OK;
    const int lp = fqa_lp(L, mode), dp = fqa_dp(d);
    FqaParams f{};
    f.g.Ah = (const uint8_t*)x_img, f.g.Wh = (const uint8_t*)qkv_hs, f.g.bias = qkv_hb, f.g.ln_in = stats;
    f.g.M = M, f.g.N = heads * 3 * dp, f.g.K = C, f.g.mode = mode;
    f.o = (float*)o_img, f.nseq = nseq, f.L = L, f.C = C, f.heads = heads, f.d = d;
    f.nseq_tile = fqa_nseq_tile(L, lp);
    if (f.nseq_tile * L > fqa_tile_rows(lp)) return fail(PAFUSE_E_SHAPE, "qkv_attention_image: %d sequences of %d tokens do not fit a tile", f.nseq_tile, L);
    f.group = group, f.group_stride = group_stride, f.seq_stride = seq_stride, f.tok_stride = tok_stride;
    f.scale = qk_scale != 0.f ? qk_scale : 1.0f / sqrtf((float)d);
    return fused_qkv_attention(f, (hipStream_t)stream);
}

int pafuse_mlp_h(const void* xh, const float* stats_in, const void* W1h, const float* bias1, const void* W2hp, const float* bias2,
                 void* out_xh, float* stats_out, int64_t M, int32_t C, float eps, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!xh || !W1h || !bias1 || !W2hp || !bias2 || !out_xh || !stats_out || M < 0) return fail(PAFUSE_E_ARG, "mlp_h: null pointer or negative M");
    if (!hmlp_has(C, 2 * C)) return fail(PAFUSE_E_SHAPE, "mlp_h: no fused MLP kernel for channel width %d (have 224, 256, 384)", C);
    MlpParams m{};
    m.g.Ah = (const uint8_t*)xh, m.g.Wh = (const uint8_t*)W2hp, m.g.bias = bias2, m.g.resid_h = (const uint8_t*)xh;
    m.g.out_xh = (uint8_t*)out_xh, m.g.ln_stats = stats_out, m.g.next_w = bias2, m.g.next_b = bias2, m.g.next_eps = eps;   // (folded: next_* only say "a LayerNorm follows")
    m.g.M = M, m.g.N = C, m.g.K = 2 * C, m.g.mode = MODE_F16X2;
    m.W1h = (const uint8_t*)W1h, m.bias1 = bias1, m.ln_in = stats_in;
    return fused_mlp(m, (hipStream_t)stream);
}

int pafuse_layernorm(const float* x, const float* w, const float* b, float* out, int64_t M, int32_t C, float eps,
                     void* stream) {
    StreamDevice on_stream_device(stream);
    if (!x || !w || !b || !out || M < 0) return fail(PAFUSE_E_ARG, "layernorm: null pointer or negative M");
    if (C <= 0 || C > 64 * LN_MAX_PER_LANE) return fail(PAFUSE_E_SHAPE, "layernorm: C=%d out of range", C);
    if (M == 0) return PAFUSE_OK;
    return launch<layernorm_kernel>("layernorm_kernel", (unsigned)((M + 3) / 4), 256, 0, (hipStream_t)stream, x, w, b, out, M, C, eps);
}

int pafuse_attention(const float* qkv, float* o, int64_t nseq, int32_t L, int32_t C, int32_t heads, int64_t group,
                     int64_t group_stride, int64_t seq_stride, int64_t tok_stride, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!qkv || !o || nseq < 0 || heads <= 0 || C % heads || group <= 0)
        return fail(PAFUSE_E_ARG, "attention: bad argument");
    AttnParams a{};
    a.qkv = qkv, a.o = o, a.nseq = nseq, a.L = L, a.C = C, a.heads = heads, a.d = C / heads;
    a.group = group, a.group_stride = group_stride, a.seq_stride = seq_stride, a.tok_stride = tok_stride;
    a.scale = 1.0f / sqrtf((float)(C / heads));
    return attention(a, (hipStream_t)stream);
}

size_t pafuse_block_workspace_bytes(int64_t rows, int32_t C) { return rows <= 0 || C <= 0 ? 0 : part_buffer_bytes(rows, C, 1, 6); }

int pafuse_block_forward(const pafuse_block_weights* w, float* x, int64_t S, int32_t L, int32_t C, int32_t heads,
                         int32_t operand_bf16, void* workspace, size_t workspace_bytes, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!w || !x || !workspace || S < 0) return fail(PAFUSE_E_ARG, "block_forward: bad argument");
    if (!mode_valid(operand_bf16)) return fail(PAFUSE_E_ARG, "block_forward: matrix-product mode %d", operand_bf16);
    if (mode_images(operand_bf16) && !hgemm_width(C)) return fail(PAFUSE_E_SHAPE, "block_forward: the image pipelines serve the widths 224 / 256 / 384");
    if (operand_bf16 == MODE_BF16X3_IMAGES && (heads <= 0 || C % heads || !w->qkv_hs || !w->qkv_hb || !xfqa_has(L, C / heads, heads)))
        return fail(PAFUSE_E_ARG, "block_forward: bf16x3 on images needs the head-major qkv image (qkv_hs, qkv_hb) and a sequence length / head "
                                  "dim with a fused qkv + attention form");
    if (mode_split(operand_bf16) && ((!w->qkv_ws && operand_bf16 != MODE_BF16X3_IMAGES) || !w->proj_ws || !w->fc1_ws || !w->fc2_ws))
        return fail(PAFUSE_E_ARG, "block_forward: split-precision mode needs the pre-split image of every linear weight");
    if (!width_supported(C)) return fail(PAFUSE_E_SHAPE, "channel width %d has no kernel", C);
    if (heads <= 0 || C % heads) return fail(PAFUSE_E_SHAPE, "block_forward: heads %d must divide C %d", heads, C);
    if (L <= 0) return fail(PAFUSE_E_SHAPE, "block_forward: sequence length %d", L);
    const int64_t M = S * L;
    if (workspace_bytes < pafuse_block_workspace_bytes(M, C)) return fail(PAFUSE_E_WORKSPACE, "workspace too small");
    if (M == 0) return PAFUSE_OK;
    hipStream_t s = (hipStream_t)stream;
    PartBuffers pb;
    carve_part((char*)workspace, M, C, 1, pb, 6);
    pb.x = x;
    // image pipelines: the qkv GEMM reads the image of LN1(x) - the fp32 rows pass through `wide` (free until qkv writes it)
    int rc = pafuse_layernorm(x, w->norm1_w, w->norm1_b, mode_images(operand_bf16) ? pb.wide : pb.xn, M, C, 1e-6f, stream);
    if (rc) return rc;
    if (operand_bf16 == MODE_F16X2 && (rc = pafuse_hsplit_rows(pb.wide, M, C, pb.xn, stream))) return rc;
    if (operand_bf16 == MODE_BF16X3_IMAGES && (rc = pafuse_xsplit_rows(pb.wide, M, C, pb.xn, stream))) return rc;
    BlockTail t{};  // plain Block.forward: no post norm, nothing after
    return run_block(*w, pb, M, C, heads, S, L, 1, L, 0, 1, t, s, false, nullptr, nullptr, operand_bf16);
}

int pafuse_time_embed(const pafuse_mixste2_weights* w, const int64_t* t, int32_t B, float* temb, float* hid_scratch,
                      void* stream) {
    StreamDevice on_stream_device(stream);
    if (!w || !t || !temb || B <= 0) return fail(PAFUSE_E_ARG, "time_embed: bad argument");
    if (w->channels % 2 || w->channels > 1024) return fail(PAFUSE_E_SHAPE, "time_embed: C=%d", w->channels);
    if (!hid_scratch) return fail(PAFUSE_E_ARG, "time_embed: null scratch");
    return launch_time_embed(w, t, 0, B, temb, hid_scratch, (hipStream_t)stream);
}

size_t pafuse_mixste2_workspace_bytes(const pafuse_mixste2_weights* w, int32_t B, int32_t P) {
    if (!w || B <= 0 || P <= 0 || w->frames <= 0 || w->joints <= 0 || w->channels <= 0) return 0;   // (a negative size must not wrap)
    return part_buffer_bytes((int64_t)B * P * w->frames * w->joints, w->channels, B, image_elem_bytes(w->operand_bf16));
}

int pafuse_mixste2_forward(const pafuse_mixste2_weights* w, const float* x2d, const float* x3d, const int64_t* t,
                           int32_t B, int32_t P, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    StreamDevice on_stream_device(stream);
    int rc = check_weights(w);
    if (rc) return rc;
    if (!x2d || !x3d || !t || !out || !workspace || B <= 0 || P <= 0)
        return fail(PAFUSE_E_ARG, "mixste2_forward: bad argument");
    if (workspace_bytes < pafuse_mixste2_workspace_bytes(w, B, P)) return fail(PAFUSE_E_WORKSPACE, "workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int64_t R = (int64_t)B * P, M = R * w->frames * w->joints;
    PartBuffers pb;
    carve_part((char*)workspace, M, w->channels, B, pb, image_elem_bytes(w->operand_bf16));
    if ((rc = launch_time_embed(w, t, 0, B, pb.temb, pb.wide, s))) return rc;
#ifdef PAFUSE_DIAG
    if (g_snap) (void)hipMemcpyAsync(g_snap + M * w->channels, pb.temb, (size_t)B * w->channels * 4, hipMemcpyDeviceToDevice, s);
#endif
    EmbedParams e{};
    e.x3d = x3d, e.x2d = x2d, e.x2d_flip = nullptr, e.joints = nullptr, e.perm = nullptr;
    e.pw = w->patch_w, e.pb = w->patch_b, e.pos = w->pos_spatial, e.temb = pb.temb;
    e.n_w = w->ste[0].norm1_w, e.n_b = w->ste[0].norm1_b, e.n_eps = 1e-6f;
    embed_outputs(e, w->operand_bf16, ln_folded(w), h_residual_only(w), pb.x, pb.xn, pb.xn, pb.stats, 0, M);
    e.B = B, e.P = P, e.F = w->frames, e.J = w->joints, e.J3 = w->joints, e.C = w->channels, e.nflip = 1;
    e.do_clamp = 0, e.scale = 1.f, e.lim = 1.1f;
    if ((rc = launch<embed_kernel>("embed_kernel", (unsigned)((M + EMBED_ROWS_PER_BLOCK - 1) / EMBED_ROWS_PER_BLOCK), 256, 0, s, e))) return rc;
    PAFUSE_TRACE(pb.temb, (size_t)B * w->channels * 4, s);
    PAFUSE_TRACE(pb.x, (size_t)M * w->channels * 4, s);
    PAFUSE_TRACE(pb.xn, (size_t)M * w->channels * 4, s);
#ifdef PAFUSE_DIAG
    if (g_snap) (void)hipMemcpyAsync(g_snap, pb.x, (size_t)M * w->channels * 4, hipMemcpyDeviceToDevice, s);
#endif
    if ((rc = run_mixste_layers(w, pb, R, s, (debug_f32_mask() & 32) != 0))) return rc;
    return launch<copy_kernel>("copy_kernel", blocks_for(M * 3), 256, 0, s, pb.pred, out, M * 3);
}

size_t pafuse_d3dp_workspace_bytes(const pafuse_d3dp_config* cfg, int32_t B, int32_t P) {
    if (!cfg || B <= 0 || P <= 0 || cfg->frames <= 0 || cfg->num_kps <= 0 || cfg->num_parts < 0 || cfg->num_parts > PAFUSE_MAX_PARTS) return 0;
    const int nflip = cfg->flip ? 2 : 1;
    size_t total = align_up((size_t)B * P * cfg->frames * cfg->num_kps * 3 * 4);  // img
    for (int i = 0; i < cfg->num_parts; ++i) {
        const pafuse_mixste2_weights& w = cfg->part[i];
        total += part_buffer_bytes((int64_t)nflip * B * P * w.frames * w.joints, w.channels, B, image_elem_bytes(w.operand_bf16));
    }
    return total + RANGE_FLAG_BYTES;   // the range flag word sits behind everything else
}

size_t pafuse_d3dp_range_flag_offset(const pafuse_d3dp_config* cfg, int32_t B, int32_t P) {
    const size_t total = pafuse_d3dp_workspace_bytes(cfg, B, P);
    return total ? total - RANGE_FLAG_BYTES : 0;
}

int pafuse_d3dp_check_range(const pafuse_d3dp_config* cfg, int32_t B, int32_t P, const void* workspace, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!cfg || !workspace || B <= 0 || P <= 0) return fail(PAFUSE_E_ARG, "d3dp_check_range: bad argument");
    int32_t flag = 0;
    const char* at = (const char*)workspace + pafuse_d3dp_range_flag_offset(cfg, B, P);
    hipError_t e = hipMemcpyAsync(&flag, at, sizeof flag, hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(PAFUSE_E_HIP, "d3dp_check_range: %s", hipGetErrorString(e));
    if (flag)
        return fail(PAFUSE_E_RANGE, "a denoiser output was not finite: in 'f16x2' an activation left the fp16 range (|a| >= 65504 makes "
                                    "its high slice inf); run this model in 'bf16x3' or 'f32' (the predictions of the affected rows are NaN)");
    return PAFUSE_OK;
}

// Side streams beside the split-precision kernels need a library WITHOUT packed-fp32 VALU instructions: on MI355X a
// v_pk_{add,mul,fma}_f32 whose src1 takes the high register of its pair for the low result (op_sel:[0,1,..]) returns wrong
// lanes while a wave of another kernel on the same SIMD issues v_mfma_f32_32x32x16_bf16 (two-kernel reproducer:
// tools/mfma_queue_isolate.hip V9.3 / V9.9 / V9.10 / V9.12; profiles/r03_bf16_mfma_concurrency.md).  hipcc's SLP vectoriser
// emits that form in the VALU-only kernels of this file (embed, LayerNorm, epilogues); __graft_entry__.build() therefore
// compiles the device code with the packed-fp32-ops target feature off and says so with -DPAFUSE_NO_PACKED_F32.  A build
// without that promise keeps the bf16-MFMA modes on the caller's stream.
static bool lanes_allowed(const pafuse_d3dp_config* cfg) {
#if defined(PAFUSE_NO_PACKED_F32) || defined(PAFUSE_ALLOW_BF16_LANES)
    (void)cfg;
    return true;
#else
    for (int i = 0; i < cfg->num_parts; ++i)
        if (cfg->part[i].operand_bf16 != MODE_F32) return false;
    return true;
#endif
}

static int d3dp_check(const pafuse_d3dp_config* cfg, int B, int P) {
    if (!cfg || B <= 0 || P <= 0) return fail(PAFUSE_E_ARG, "d3dp: bad argument");
    if (cfg->num_parts < 1 || cfg->num_parts > PAFUSE_MAX_PARTS) return fail(PAFUSE_E_SHAPE, "num_parts %d", cfg->num_parts);
    int total = 0;
    for (int i = 0; i < cfg->num_parts; ++i) {
        int rc = check_weights(&cfg->part[i]);
        if (rc) return rc;
        if (cfg->part[i].frames != cfg->frames) return fail(PAFUSE_E_SHAPE, "part %d: frames mismatch", i);
        if (!cfg->part_joints[i]) return fail(PAFUSE_E_ARG, "part %d: null joint list", i);
        total += cfg->part[i].joints;
    }
    if (total != cfg->num_kps) return fail(PAFUSE_E_SHAPE, "parts cover %d joints, expected %d", total, cfg->num_kps);
    if (!cfg->joint_part || !cfg->joint_local || (cfg->flip && !cfg->flip_perm))
        return fail(PAFUSE_E_ARG, "d3dp: null index table");
    return PAFUSE_OK;
}

// The loop behind pafuse_d3dp_sample (key4 null: the draws are read from `noise`) and pafuse_d3dp_sample_seeded (key4 set: the
// draws are generated where they are consumed, noise stream v1; `noise` is null).
static int d3dp_sample_impl(const pafuse_d3dp_config* cfg, const pafuse_ddim_step* steps, int32_t nsteps, const float* x2d,
                            const float* x2d_flip, const float* noise, int32_t n_draws, const uint32_t* key4, int32_t B, int32_t P,
                            float* out, void* workspace, size_t workspace_bytes, void* stream, void* const* aux_streams,
                            int32_t n_aux) {
    StreamDevice on_stream_device(stream);
    int rc = d3dp_check(cfg, B, P);
    if (rc) return rc;
    if (!steps || nsteps <= 0 || !x2d || !(noise || key4) || !out || !workspace || (cfg->flip && !x2d_flip) || (!key4 && n_draws < 1))
        return fail(PAFUSE_E_ARG, "d3dp_sample: bad argument");
    int need = 1;
    for (int k = 0; k < nsteps; ++k) need += steps[k].last ? 0 : 1;
    if (!key4 && n_draws < need) return fail(PAFUSE_E_ARG, "d3dp_sample: %d noise draws given, %d needed", n_draws, need);
    if (workspace_bytes < pafuse_d3dp_workspace_bytes(cfg, B, P)) return fail(PAFUSE_E_WORKSPACE, "workspace too small");

    hipStream_t s0 = (hipStream_t)stream;
    const int nflip = cfg->flip ? 2 : 1, F = cfg->frames, J = cfg->num_kps, NP = cfg->num_parts;
    const int64_t R = (int64_t)nflip * B * P;
    const int64_t img_elems = (int64_t)B * P * F * J * 3;
    char* base = (char*)workspace;
    float* img = (float*)base;
    base += align_up((size_t)img_elems * 4);
    PartBuffers pb[PAFUSE_MAX_PARTS];
    for (int i = 0; i < NP; ++i)
        base = carve_part(base, R * F * cfg->part[i].joints, cfg->part[i].channels, B, pb[i], image_elem_bytes(cfg->part[i].operand_bf16));
    int32_t* const range_flag = reinterpret_cast<int32_t*>((char*)workspace + pafuse_d3dp_range_flag_offset(cfg, B, P));
    if (hipMemsetAsync(range_flag, 0, sizeof(int32_t), s0) != hipSuccess) return fail(PAFUSE_E_HIP, "d3dp_sample: memset failed");

    // Parts are independent inside a step, and so are hypotheses: with aux streams the work of a step is cut into
    // (part, hypothesis-group) lanes, each a chain of small launches on its own stream, so that the ramp-up and
    // tail of one lane's kernels are filled by the other lanes (groups = (n_aux + 1) / parts, at least 1).
    // Without aux streams (or in a build that may hold packed-fp32 instructions, see lanes_allowed) everything runs on
    // `stream`, block k of every part in shared grids.
    n_aux = lanes_allowed(cfg) ? n_aux : 0;
    const int n_lanes_max = 1 + (n_aux > 0 ? n_aux : 0);
    int groups = n_lanes_max / NP;
    if (groups < 1) groups = 1;
    if (groups > R) groups = (int)R;
    const int lanes = NP * groups;
    auto lane_stream = [&](int lane) -> hipStream_t {
        if (n_aux <= 0 || lane == 0) return s0;
        return (hipStream_t)aux_streams[(lane - 1) % n_aux];
    };
    const bool multi = n_aux > 0 && lanes > 1;
    constexpr int MAX_LANES = 64;
    if (lanes > MAX_LANES) return fail(PAFUSE_E_ARG, "too many stream lanes (%d)", lanes);
    if (key4) {
        if ((rc = launch<noise_fill_kernel>("noise_fill_kernel", blocks_for(img_elems / 3), 256, 0, s0, key4, 0, B, P, F, J, img))) return rc;
    } else {
        if ((rc = launch<copy_kernel>("copy_kernel", blocks_for(img_elems), 256, 0, s0, noise, img, img_elems))) return rc;
    }
    hipEvent_t ev_fork = nullptr, ev_join[MAX_LANES] = {};
    if (multi) {
        hipError_t e = hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming);
        for (int i = 1; i < lanes && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev_join[i], hipEventDisableTiming);
        if (e != hipSuccess) {
            if (ev_fork) hipEventDestroy(ev_fork);
            for (int i = 1; i < lanes; ++i)
                if (ev_join[i]) hipEventDestroy(ev_join[i]);
            return fail(PAFUSE_E_HIP, "hipEventCreate: %s", hipGetErrorString(e));
        }
    }
    bool forked = false;  // lanes hold work the main stream has not waited for yet
    hipError_t sync_err = hipSuccess;  // first failing event call: a missed fork/join would be a silent race
    auto note = [&](hipError_t e) {
        if (e != hipSuccess && sync_err == hipSuccess) sync_err = e;
    };
    auto join = [&]() {
        for (int i = 1; i < lanes; ++i) {
            note(hipEventRecord(ev_join[i], lane_stream(i)));
            note(hipStreamWaitEvent(s0, ev_join[i], 0));
        }
        forked = false;
    };
    int draw = 1;
    for (int k = 0; k < nsteps && rc == PAFUSE_OK; ++k) {
        const pafuse_ddim_step& st = steps[k];
        // the time embedding of every part once, on the main stream, before the fork
        for (int i = 0; i < NP && rc == PAFUSE_OK; ++i)
            rc = launch_time_embed(&cfg->part[i], nullptr, st.time, B, pb[i].temb, pb[i].wide, s0);
        if (rc) break;
        if (multi) {
            note(hipEventRecord(ev_fork, s0));
            for (int i = 1; i < lanes; ++i) note(hipStreamWaitEvent(lane_stream(i), ev_fork, 0));
            forked = true;
            if (sync_err != hipSuccess) {
                rc = fail(PAFUSE_E_HIP, "d3dp_sample: stream fork failed: %s", hipGetErrorString(sync_err));
                break;
            }
        }
        const bool together = !multi && parts_groupable(cfg);  // one stream: block k of every part in shared grids
        for (int lane = 0; lane < lanes && rc == PAFUSE_OK; ++lane) {
            const int i = lane % NP, gi = lane / NP;
            const pafuse_mixste2_weights* w = &cfg->part[i];
            hipStream_t ls = lane_stream(lane);
            const int64_t r0 = R * gi / groups, r1 = R * (gi + 1) / groups;
            const int64_t rows_per_r = (int64_t)F * w->joints, row0 = r0 * rows_per_r, nrows = (r1 - r0) * rows_per_r;
            EmbedParams e{};
            e.x3d = img, e.x2d = x2d, e.x2d_flip = x2d_flip, e.joints = cfg->part_joints[i], e.perm = cfg->flip_perm;
            e.pw = w->patch_w, e.pb = w->patch_b, e.pos = w->pos_spatial, e.temb = pb[i].temb;
            e.n_w = w->ste[0].norm1_w, e.n_b = w->ste[0].norm1_b, e.n_eps = 1e-6f;
            // (the statistics go where offset_rows puts this group's; rows and image are indexed by the absolute row)
            embed_outputs(e, w->operand_bf16, ln_folded(w), h_residual_only(w), pb[i].x, pb[i].xn, pb[i].xn,
                          ln_folded(w) ? pb[i].stats + row0 * 2 : nullptr, row0, nrows);
            e.B = B, e.P = P, e.F = F, e.J = w->joints, e.J3 = J, e.C = w->channels, e.nflip = nflip;
            e.do_clamp = 1, e.scale = (float)cfg->scale, e.lim = (float)(1.1 * cfg->scale);
            if ((rc = launch<embed_kernel>("embed_kernel", (unsigned)((nrows + EMBED_ROWS_PER_BLOCK - 1) / EMBED_ROWS_PER_BLOCK), 256, 0, ls, e))) break;
            if (!together) rc = run_mixste_layers(w, offset_rows(pb[i], row0, w->channels), r1 - r0, ls);
        }
        if (rc) break;
        if (together) {
            const pafuse_mixste2_weights* ws[PAFUSE_MAX_PARTS];
            int64_t Rs[PAFUSE_MAX_PARTS];
            for (int i = 0; i < NP; ++i) ws[i] = &cfg->part[i], Rs[i] = R;
            if ((rc = run_mixste_layers_n(ws, pb, Rs, NP, s0))) break;
        }
        if (multi) {
            join();
            if (sync_err != hipSuccess) {
                rc = fail(PAFUSE_E_HIP, "d3dp_sample: stream join failed: %s", hipGetErrorString(sync_err));
                break;
            }
        }
        FinalizeParams f{};
        for (int i = 0; i < NP; ++i) f.pred[i] = pb[i].pred, f.Jp[i] = cfg->part[i].joints;
        f.joint_part = cfg->joint_part, f.joint_local = cfg->joint_local, f.perm = cfg->flip_perm;
        f.img = img, f.noise = (st.last || key4) ? nullptr : noise + (int64_t)draw * img_elems, f.out = out;
        f.key4 = key4, f.draw = draw;
        f.B = B, f.P = P, f.F = F, f.J = J, f.T = nsteps, f.step = k, f.flip = cfg->flip, f.last = st.last;
        f.scale = (float)cfg->scale, f.lim = (float)(1.1 * cfg->scale), f.sr = st.sqrt_recip_acp, f.srm1 = st.sqrt_recipm1_acp, f.c = st.c;
        f.an_f = (float)st.sqrt_alpha_next, f.c_f = (float)st.c, f.sigma_f = (float)st.sigma;
        f.range_flag = range_flag;
        const int64_t n = (int64_t)B * P * F * J;
        rc = key4 ? launch<finalize_seeded_kernel>("finalize_kernel", blocks_for(n), 256, 0, s0, f)
                  : launch<finalize_kernel>("finalize_kernel", blocks_for(n), 256, 0, s0, f);
        if (!st.last) ++draw;
    }
    if (multi) {
        if (forked) join();  // error exit mid-step: the caller's stream still orders after everything launched
        // aux streams beyond the lanes in use did no work: nothing to join (callers that capture the call into a graph
        // must fork only the first pafuse_d3dp_lanes(...) - 1 aux streams, see include/pafuse_hip.h)
        hipEventDestroy(ev_fork);
        for (int i = 1; i < lanes; ++i) hipEventDestroy(ev_join[i]);
        if (rc == PAFUSE_OK && sync_err != hipSuccess)
            rc = fail(PAFUSE_E_HIP, "d3dp_sample: stream join failed: %s", hipGetErrorString(sync_err));
    }
    return rc;
}

int pafuse_d3dp_sample(const pafuse_d3dp_config* cfg, const pafuse_ddim_step* steps, int32_t nsteps, const float* x2d,
                       const float* x2d_flip, const float* noise, int32_t n_draws, int32_t B, int32_t P, float* out,
                       void* workspace, size_t workspace_bytes, void* stream, void* const* aux_streams, int32_t n_aux) {
    return d3dp_sample_impl(cfg, steps, nsteps, x2d, x2d_flip, noise, n_draws, nullptr, B, P, out, workspace, workspace_bytes, stream,
                            aux_streams, n_aux);
}

int pafuse_d3dp_sample_seeded(const pafuse_d3dp_config* cfg, const pafuse_ddim_step* steps, int32_t nsteps, const float* x2d,
                              const float* x2d_flip, const uint32_t* key4_dev, int32_t B, int32_t P, float* out, void* workspace,
                              size_t workspace_bytes, void* stream, void* const* aux_streams, int32_t n_aux) {
    if (!key4_dev) return fail(PAFUSE_E_ARG, "d3dp_sample_seeded: null key");
    return d3dp_sample_impl(cfg, steps, nsteps, x2d, x2d_flip, nullptr, 0, key4_dev, B, P, out, workspace, workspace_bytes, stream,
                            aux_streams, n_aux);
}

int pafuse_noise_fill(const uint32_t* key4_dev, int32_t draw, int32_t B, int32_t P, int32_t F, int32_t J, float* out, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!key4_dev || !out) return fail(PAFUSE_E_ARG, "noise_fill: null pointer");
    if (draw < 0 || B <= 0 || P <= 0 || F <= 0 || J <= 0) return fail(PAFUSE_E_ARG, "noise_fill: bad size (draw=%d B=%d P=%d F=%d J=%d)", draw, B, P, F, J);
    const int64_t n = (int64_t)B * P * F * J, blocks = (n + 255) / 256;
    if ((int64_t)F * J > 0xffffffffLL || blocks > 0x7fffffff) return fail(PAFUSE_E_ARG, "noise_fill: size out of range");
    return launch<noise_fill_kernel>("noise_fill_kernel", (unsigned)blocks, 256, 0, (hipStream_t)stream, key4_dev, draw, B, P, F, J, out);
}

int pafuse_d3dp_lanes(const pafuse_d3dp_config* cfg, int32_t B, int32_t P, int32_t n_aux) {
    if (!cfg || B <= 0 || P <= 0 || cfg->num_parts < 1) return fail(PAFUSE_E_ARG, "d3dp_lanes: bad argument");
    if (!lanes_allowed(cfg)) return 1;
    const int64_t R = (int64_t)(cfg->flip ? 2 : 1) * B * P;
    int groups = (1 + (n_aux > 0 ? n_aux : 0)) / cfg->num_parts;
    if (groups < 1) groups = 1;
    if (groups > R) groups = (int)R;
    const int lanes = cfg->num_parts * groups;
    if (n_aux <= 0) return 1;
    return lanes < 1 + n_aux ? lanes : 1 + n_aux;  // distinct streams in use (lane 0 = the caller's stream)
}

// operands shared by pafuse_embed and pafuse_embed_unit, checked before anything is launched; fills the input side of `e`
static int embed_inputs(EmbedParams& e, const float* x3d, const float* x2d, const float* x2d_flip, const int32_t* joints,
                        const int32_t* perm, const float* patch_w, const float* patch_b, const float* pos_spatial, const float* temb,
                        const float* norm_w, const float* norm_b, float norm_eps, int B, int P, int F, int J, int J3, int C, int nflip,
                        int do_clamp, double scale) {
    if (!x3d || !x2d || !patch_w || !patch_b || !pos_spatial || !temb || !norm_w || !norm_b)
        return fail(PAFUSE_E_ARG, "embed: null pointer");
    if (B <= 0 || P <= 0 || F <= 0 || J <= 0 || J3 < J || (nflip != 1 && nflip != 2))
        return fail(PAFUSE_E_ARG, "embed: bad size (B=%d P=%d F=%d J=%d J3=%d nflip=%d)", B, P, F, J, J3, nflip);
    if (nflip == 2 && (!x2d_flip || !perm)) return fail(PAFUSE_E_ARG, "embed: the flipped half needs x2d_flip and perm");
    if (J3 != J && !joints) return fail(PAFUSE_E_ARG, "embed: a part of %d joints out of %d needs its joint list", J, J3);
    if (C % 4 || C <= 0 || C > EMBED_NV * 128) return fail(PAFUSE_E_SHAPE, "embed: C=%d (need %%4, <= %d)", C, EMBED_NV * 128);
    if (do_clamp && !(scale > 0.0)) return fail(PAFUSE_E_ARG, "embed: scale must be positive");
    e.x3d = x3d, e.x2d = x2d, e.x2d_flip = x2d_flip, e.joints = joints, e.perm = perm;
    e.pw = patch_w, e.pb = patch_b, e.pos = pos_spatial, e.temb = temb;
    e.n_w = norm_w, e.n_b = norm_b, e.n_eps = norm_eps;
    e.B = B, e.P = P, e.F = F, e.J = J, e.J3 = J3, e.C = C, e.nflip = nflip, e.do_clamp = do_clamp;
    e.scale = (float)scale, e.lim = (float)(1.1 * scale);
    return PAFUSE_OK;
}

static int launch_embed(const EmbedParams& e, hipStream_t s) {
    const int64_t blocks = (e.nrows + EMBED_ROWS_PER_BLOCK - 1) / EMBED_ROWS_PER_BLOCK;
    if (blocks > 0x7fffffff) return fail(PAFUSE_E_ARG, "embed: grid out of range");
    return launch<embed_kernel>("embed_kernel", (unsigned)blocks, 256, 0, s, e);
}

int pafuse_embed(const float* x3d, const float* x2d, const float* x2d_flip, const int32_t* joints, const int32_t* perm,
                 const float* patch_w, const float* patch_b, const float* pos_spatial, const float* temb,
                 const float* norm_w, const float* norm_b, float norm_eps, int32_t B, int32_t P, int32_t F, int32_t J,
                 int32_t J3, int32_t C, int32_t nflip, int32_t do_clamp, double scale, float* x, float* xn, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!x || !xn) return fail(PAFUSE_E_ARG, "embed: null pointer");
    EmbedParams e{};
    if (int rc = embed_inputs(e, x3d, x2d, x2d_flip, joints, perm, patch_w, patch_b, pos_spatial, temb, norm_w, norm_b, norm_eps, B, P,
                              F, J, J3, C, nflip, do_clamp, scale))
        return rc;
    embed_outputs(e, MODE_F32, false, false, x, xn, nullptr, nullptr, 0, (int64_t)nflip * B * P * F * J);
    return launch_embed(e, (hipStream_t)stream);
}

int pafuse_embed_unit(const pafuse_embed_args* a, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!a) return fail(PAFUSE_E_ARG, "embed_unit: null arguments");
    EmbedParams e{};
    if (int rc = embed_inputs(e, a->x3d, a->x2d, a->x2d_flip, a->joints, a->perm, a->patch_w, a->patch_b, a->pos_spatial, a->temb,
                              a->norm_w, a->norm_b, a->norm_eps, a->B, a->P, a->F, a->J, a->J3, a->C, a->nflip, a->do_clamp, a->scale))
        return rc;
    const int mode = a->operand_bf16;
    if (!mode_valid(mode)) return fail(PAFUSE_E_ARG, "embed_unit: matrix-product mode %d", mode);
    const bool folded = a->ln_folded != 0, h_only = a->h_residual_only != 0, img = mode_images(mode);
    if (folded && !mode_split(mode)) return fail(PAFUSE_E_ARG, "embed_unit: the folded LayerNorm exists in the split-precision modes only");
    if (h_only && !(img && folded)) return fail(PAFUSE_E_ARG, "embed_unit: the H-residual-only form is an image pipeline with the LayerNorm folded");
    const int64_t M = (int64_t)a->nflip * a->B * a->P * a->F * a->J;
    if (a->row0 < 0 || a->nrows < 1 || a->row0 > M - a->nrows)
        return fail(PAFUSE_E_ARG, "embed_unit: rows [%lld, %lld + %lld) outside the %lld rows of the token matrix", (long long)a->row0,
                    (long long)a->row0, (long long)a->nrows, (long long)M);
    if (img && a->C % (mode == MODE_BF16X3_IMAGES ? 32 : 8))
        return fail(PAFUSE_E_SHAPE, "embed_unit: C=%d: an %s image has rows of whole %d-element blocks", a->C,
                    mode == MODE_BF16X3_IMAGES ? "X" : "H", mode == MODE_BF16X3_IMAGES ? 32 : 8);
    if (!h_only && !a->x) return fail(PAFUSE_E_ARG, "embed_unit: no x");
    if (img && !a->image) return fail(PAFUSE_E_ARG, "embed_unit: mode %d writes an image: no image", mode);
    if (!img && !folded && !a->xn) return fail(PAFUSE_E_ARG, "embed_unit: no xn");
    if (folded && !a->stats) return fail(PAFUSE_E_ARG, "embed_unit: the folded LayerNorm writes statistics: no stats");
    embed_outputs(e, mode, folded, h_only, a->x, a->xn, a->image, a->stats, a->row0, a->nrows);
    return launch_embed(e, (hipStream_t)stream);
}

int pafuse_ddim_finalize(const float* const* pred, const int32_t* part_joints, int32_t num_parts, const int32_t* joint_part,
                         const int32_t* joint_local, const int32_t* flip_perm, float* img, const float* noise, float* out,
                         int32_t B, int32_t P, int32_t F, int32_t J, int32_t T, int32_t step, int32_t flip, double scale,
                         const pafuse_ddim_step* st, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!pred || !part_joints || !joint_part || !joint_local || !img || !out || !st)
        return fail(PAFUSE_E_ARG, "ddim_finalize: null pointer");
    if (num_parts < 1 || num_parts > PAFUSE_MAX_PARTS) return fail(PAFUSE_E_SHAPE, "ddim_finalize: num_parts %d", num_parts);
    if (B <= 0 || P <= 0 || F <= 0 || J <= 0 || T <= 0 || step < 0 || step >= T)
        return fail(PAFUSE_E_ARG, "ddim_finalize: bad size");
    if (flip && !flip_perm) return fail(PAFUSE_E_ARG, "ddim_finalize: flip needs the permutation");
    if (!st->last && !noise) return fail(PAFUSE_E_ARG, "ddim_finalize: an update step needs its noise draw");
    FinalizeParams f{};
    int total = 0;
    for (int i = 0; i < num_parts; ++i) {
        if (!pred[i] || part_joints[i] <= 0) return fail(PAFUSE_E_ARG, "ddim_finalize: part %d", i);
        f.pred[i] = pred[i], f.Jp[i] = part_joints[i], total += part_joints[i];
    }
    if (total != J) return fail(PAFUSE_E_SHAPE, "ddim_finalize: parts cover %d joints, expected %d", total, J);
    f.joint_part = joint_part, f.joint_local = joint_local, f.perm = flip_perm;
    f.img = img, f.noise = st->last ? nullptr : noise, f.out = out;
    f.B = B, f.P = P, f.F = F, f.J = J, f.T = T, f.step = step, f.flip = flip ? 1 : 0, f.last = st->last;
    f.scale = (float)scale, f.lim = (float)(1.1 * scale), f.sr = st->sqrt_recip_acp, f.srm1 = st->sqrt_recipm1_acp, f.c = st->c;
    f.an_f = (float)st->sqrt_alpha_next, f.c_f = (float)st->c, f.sigma_f = (float)st->sigma;
    const int64_t n = (int64_t)B * P * F * J;
    return launch<finalize_kernel>("finalize_kernel", blocks_for(n), 256, 0, (hipStream_t)stream, f);
}

int pafuse_hypothesis_errors(const float* pred, const float* gt, const float* x2d, const float* traj, const float* cam,
                             const int32_t* conn, const int32_t* pbroot, int32_t B, int32_t T, int32_t P, int32_t F,
                             int32_t J, float* e3, float* epb, float* jbest, float* pagg, float* jagg, float* paggpb,
                             void* stream) {
    StreamDevice on_stream_device(stream);
    if (!pred || !gt || !x2d || !traj || !cam || !conn || !pbroot || !e3 || !epb || !jbest || !pagg || !jagg || !paggpb)
        return fail(PAFUSE_E_ARG, "hypothesis_errors: null pointer");
    if (B <= 0 || T <= 0 || P <= 0 || F <= 0 || J <= 0) return fail(PAFUSE_E_ARG, "hypothesis_errors: bad size");
    MetricsParams m{};
    m.pred = pred, m.gt = gt, m.x2d = x2d, m.traj = traj, m.cam = cam, m.conn = conn, m.pbroot = pbroot;
    m.e3 = e3, m.epb = epb, m.jbest = jbest, m.pagg = pagg, m.jagg = jagg, m.paggpb = paggpb;
    m.B = B, m.T = T, m.P = P, m.F = F, m.J = J;
    const int64_t n = (int64_t)B * T * F * J;
    return launch<metrics_kernel>("metrics_kernel", blocks_for(n), 256, 0, (hipStream_t)stream, m);
}

// ---- what the partial-state entries below share (their layouts: the views structs of kernels.hpp) ----
// the prologue of a partials entry: the state buffer holds the `need` bytes the entry writes, 8-byte aligned
static int check_state(const char* who, const void* state, size_t state_bytes, size_t need) {
    if (need && (!state || state_bytes < need)) return fail(PAFUSE_E_ARG, "%s: the state needs %zu bytes", who, need);
    if ((uintptr_t)state % 8) return fail(PAFUSE_E_ARG, "%s: the state must be 8-byte aligned", who);
    return PAFUSE_OK;
}

// what of its operands the merged state of a combine may lie over
enum class MergeOver { Unchecked, Nothing, First };

// the prologue of a combine entry: W states of `head` bytes, `stride` bytes apart, every pointer 8-byte aligned; where the
// merged state may lie; the grid
static int check_combine(const char* who, const void* states, int32_t W, size_t stride, size_t head, const void* merged,
                         MergeOver over, int64_t blocks) {
    if (stride < head || stride % 8 || (uintptr_t)states % 8 || (uintptr_t)merged % 8)
        return fail(PAFUSE_E_ARG, "%s: states are %zu bytes or more apart, 8-byte aligned", who, head);
    const char *lo = (const char*)states, *mg = (const char*)merged;
    if (merged && over == MergeOver::Nothing && mg < lo + (size_t)W * stride && mg + head > lo)
        return fail(PAFUSE_E_ARG, "%s: a merge over its own operands cannot also write the maps", who);
    if (merged && over == MergeOver::First && mg != lo && mg < lo + (size_t)(W - 1) * stride + head && mg + head > lo)
        return fail(PAFUSE_E_ARG, "%s: of its operands the merged state may only lie over the first", who);
    if (blocks > 0x7fffffff) return fail(PAFUSE_E_ARG, "%s: grid out of range", who);
    return PAFUSE_OK;
}

// the neutral states (what an empty shard writes; no kernel runs): zero sums, +inf minima, no candidate
static int neutral_state(const char* who, const PartialsStateViews& v, int64_t n, size_t hsum_bytes, hipStream_t s) {
    hipError_t e = hipSuccess;
    if (n) {
        e = hipMemsetAsync(v.sum, 0, (size_t)n * 3 * sizeof(double), s);
        if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)v.jbest, 0x7f800000, (size_t)n, s);
        if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)v.e2, 0x7f800000, (size_t)n, s);
        if (e == hipSuccess) e = hipMemsetAsync(v.sel3, 0, (size_t)n * 4, s);
        if (e == hipSuccess) e = hipMemsetAsync(v.idx, 0xff, (size_t)n * 4, s);
    }
    if (e == hipSuccess && hsum_bytes) e = hipMemsetAsync(v.hsum, 0, hsum_bytes, s);
    if (e != hipSuccess) return fail(PAFUSE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    return PAFUSE_OK;
}

// (+inf, -1, NaN NaN NaN); Views: PoseStateViews or FramePoseViews, which name these four fields alike
extern "C++" template <class Views>
static int neutral_state(const char* who, const Views& v, int64_t n, hipStream_t s) {
    hipError_t e = hipSuccess;
    if (n) {
        e = hipMemsetAsync(v.sum, 0, (size_t)n * 3 * sizeof(double), s);
        if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)v.e2, 0x7f800000, (size_t)n, s);
        if (e == hipSuccess) e = hipMemsetAsync(v.idx, 0xff, (size_t)n * 4, s);
        if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)v.sel, 0x7fc00000, (size_t)n * 3, s);
    }
    if (e != hipSuccess) return fail(PAFUSE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    return PAFUSE_OK;
}

// (+inf, -1, 0)
static int neutral_state(const char* who, const P2StateViews& v, int64_t n, size_t psum_bytes, hipStream_t s) {
    hipError_t e = hipSuccess;
    if (n) {
        e = hipMemsetD32Async((hipDeviceptr_t)v.jbest, 0x7f800000, (size_t)n, s);
        if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)v.e2, 0x7f800000, (size_t)n, s);
        if (e == hipSuccess) e = hipMemsetAsync(v.sel, 0, (size_t)n * 4, s);
        if (e == hipSuccess) e = hipMemsetAsync(v.idx, 0xff, (size_t)n * 4, s);
    }
    if (e == hipSuccess && psum_bytes) e = hipMemsetAsync(v.psum, 0, psum_bytes, s);
    if (e != hipSuccess) return fail(PAFUSE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    return PAFUSE_OK;
}

static bool partials_sizes_ok(int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J, int32_t num_parts) {
    return B >= 0 && T > 0 && P_r >= 0 && F > 0 && J > 0 && num_parts >= 1 && num_parts <= PAFUSE_MAX_PARTS;
}
static int partials_nblk(int32_t F, int32_t J) { return (int)(((int64_t)F * J + 255) / 256); }

size_t pafuse_hypothesis_partials_bytes(int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J, int32_t num_parts) {
    if (!partials_sizes_ok(B, T, P_r, F, J, num_parts)) return 0;
    return PartialsStateViews::head_bytes((int64_t)B * T * F * J) + (size_t)P_r * T * (1 + num_parts) * 8;
}

size_t pafuse_hypothesis_partials_workspace_bytes(int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J, int32_t num_parts) {
    if (!partials_sizes_ok(B, T, P_r, F, J, num_parts)) return 0;
    return (size_t)B * T * partials_nblk(F, J) * P_r * (1 + num_parts) * 8;
}

int pafuse_hypothesis_partials(const float* pred, const float* gt, const float* x2d, const float* traj, const float* cam,
                               const int32_t* conn, const int32_t* pbroot, const int32_t* part, int32_t num_parts, int32_t B,
                               int32_t T, int32_t P_r, int32_t F, int32_t J, int32_t h0, void* state, size_t state_bytes,
                               void* workspace, size_t workspace_bytes, void* stream) {
    StreamDevice on_stream_device(stream);
    if (num_parts < 1 || num_parts > PAFUSE_MAX_PARTS) return fail(PAFUSE_E_SHAPE, "hypothesis_partials: num_parts %d", num_parts);
    if (B < 0 || T <= 0 || P_r < 0 || F <= 0 || J <= 0 || h0 < 0) return fail(PAFUSE_E_ARG, "hypothesis_partials: bad size");
    if (int rc = check_state("hypothesis_partials", state, state_bytes, pafuse_hypothesis_partials_bytes(B, T, P_r, F, J, num_parts))) return rc;
    const int64_t n = (int64_t)B * T * F * J;
    const PartialsStateViews v(state, n);
    hipStream_t s = (hipStream_t)stream;
    if (B == 0 || P_r == 0) return neutral_state("hypothesis_partials", v, n, (size_t)P_r * T * (1 + num_parts) * 8, s);
    if (!pred || !gt || !x2d || !traj || !cam || !conn || !pbroot || !part)
        return fail(PAFUSE_E_ARG, "hypothesis_partials: null pointer");
    const size_t wneed = pafuse_hypothesis_partials_workspace_bytes(B, T, P_r, F, J, num_parts);
    if (!workspace || workspace_bytes < wneed || (uintptr_t)workspace % 8)
        return fail(PAFUSE_E_WORKSPACE, "hypothesis_partials: the workspace needs %zu bytes, 8-byte aligned", wneed);
    PartialsParams m{};
    m.pred = pred, m.gt = gt, m.x2d = x2d, m.traj = traj, m.cam = cam, m.conn = conn, m.pbroot = pbroot, m.part = part;
    m.st = v, m.share = (double*)workspace;
    m.B = B, m.T = T, m.P = P_r, m.F = F, m.J = J, m.h0 = h0, m.nv = 1 + num_parts, m.nblk = partials_nblk(F, J);
    const int64_t blocks = (int64_t)B * T * m.nblk;
    if (blocks > 0x7fffffff || (int64_t)P_r * T > 0x7fffffff || (int64_t)B * m.nblk > 0x7fffffff)
        return fail(PAFUSE_E_ARG, "hypothesis_partials: grid out of range");
    int rc = launch<partials_kernel>("partials_kernel", (unsigned)blocks, 256, 0, s, m);
    if (rc) return rc;
    PartialsHsumParams r{};
    r.share = m.share, r.hsum = v.hsum, r.B = B, r.T = T, r.P = P_r, r.nv = m.nv, r.nblk = m.nblk;
    return launch<partials_hsum_kernel>("partials_hsum_kernel", (unsigned)((int64_t)P_r * T), 256, 0, s, r);
}

int pafuse_hypothesis_combine(const void* states, int32_t W, size_t stride_bytes, const float* gt, const int32_t* conn,
                              const int32_t* pbroot, int32_t B, int32_t T, int32_t F, int32_t J, int32_t P_total, void* merged,
                              float* jbest, float* pagg, float* jagg, float* paggpb, void* stream) {
    StreamDevice on_stream_device(stream);
    if (B < 0 || T <= 0 || F <= 0 || J <= 0 || W < 1) return fail(PAFUSE_E_ARG, "hypothesis_combine: bad size");
    const bool maps = jbest || pagg || jagg || paggpb;
    if (maps && !(jbest && pagg && jagg && paggpb)) return fail(PAFUSE_E_ARG, "hypothesis_combine: the four maps come together");
    if (!maps && !merged) return fail(PAFUSE_E_ARG, "hypothesis_combine: nothing to write");
    if (maps && P_total < 1) return fail(PAFUSE_E_ARG, "hypothesis_combine: P_total %d", P_total);
    const int64_t n = (int64_t)B * T * F * J;
    if (n == 0) return PAFUSE_OK;
    if (!states || !gt || !conn || !pbroot) return fail(PAFUSE_E_ARG, "hypothesis_combine: null pointer");
    if (int rc = check_combine("hypothesis_combine", states, W, stride_bytes, PartialsStateViews::head_bytes(n), merged,
                               maps ? MergeOver::Nothing : MergeOver::Unchecked, (n + 255) / 256)) return rc;
    CombineParams c{};
    c.states = (const char*)states, c.stride = (int64_t)stride_bytes, c.W = W, c.gt = gt, c.conn = conn, c.pbroot = pbroot;
    if (merged) c.merged = PartialsStateViews(merged, n);
    c.jbest = jbest, c.pagg = pagg, c.jagg = jagg, c.paggpb = paggpb;
    c.B = B, c.T = T, c.F = F, c.J = J, c.P = P_total;
    return launch<combine_kernel>("combine_kernel", blocks_for(n), 256, 0, (hipStream_t)stream, c);
}

// state of pafuse_pose_partials: double sum[n][3] | float e2[n] | int32 idx[n] | float sel[n][3], rounded up to 8 bytes
size_t pafuse_pose_partials_bytes(int32_t B, int32_t T, int32_t F, int32_t J) {
    if (B < 0 || T <= 0 || F <= 0 || J <= 0) return 0;
    return PoseStateViews::bytes((int64_t)B * T * F * J);
}

int pafuse_pose_partials(const float* pred, const float* x2d, const float* traj, const float* cam, const int32_t* conn,
                         int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J, int32_t h0, void* state, size_t state_bytes,
                         void* stream) {
    StreamDevice on_stream_device(stream);
    if (B < 0 || T <= 0 || P_r < 0 || F <= 0 || J <= 0 || h0 < 0) return fail(PAFUSE_E_ARG, "pose_partials: bad size");
    const int given = (x2d ? 1 : 0) + (traj ? 1 : 0) + (cam ? 1 : 0);
    if (given != 0 && given != 3)
        return fail(PAFUSE_E_ARG, "pose_partials: x2d, traj and cam come together (all null: mean-only)");
    if (int rc = check_state("pose_partials", state, state_bytes, pafuse_pose_partials_bytes(B, T, F, J))) return rc;
    const int64_t n = (int64_t)B * T * F * J;
    const PoseStateViews v(state, n);
    hipStream_t s = (hipStream_t)stream;
    if (B == 0 || P_r == 0) return neutral_state("pose_partials", v, n, s);   // no kernel runs
    if (!pred || !conn) return fail(PAFUSE_E_ARG, "pose_partials: null pointer");
    if ((n + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "pose_partials: grid out of range");
    PosePartialsParams m{};
    m.pred = pred, m.x2d = x2d, m.traj = traj, m.cam = cam, m.conn = conn, m.st = v;
    m.B = B, m.T = T, m.P = P_r, m.F = F, m.J = J, m.h0 = h0;
    return launch<pose_partials_kernel>("pose_partials_kernel", blocks_for(n), 256, 0, s, m);
}

// pafuse_pose_partials without a trajectory: the root of every (hypothesis, frame) is fitted from x2d, conf and the
// intrinsics (pose_fit_partials_kernel); the state is the one above
int pafuse_pose_partials_fit(const float* pred, const float* x2d, const float* conf, const float* cam, const int32_t* conn,
                             int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J, int32_t h0, void* state,
                             size_t state_bytes, float* tfit, void* stream) {
    StreamDevice on_stream_device(stream);
    if (B < 0 || T <= 0 || P_r < 0 || F <= 0 || J <= 0 || h0 < 0) return fail(PAFUSE_E_ARG, "pose_partials_fit: bad size");
    if (!x2d || !cam) return fail(PAFUSE_E_ARG, "pose_partials_fit: x2d and cam are needed (conf may be null: every weight 1)");
    if (int rc = check_state("pose_partials_fit", state, state_bytes, pafuse_pose_partials_bytes(B, T, F, J))) return rc;
    const int64_t n = (int64_t)B * T * F * J;
    const PoseStateViews v(state, n);
    hipStream_t s = (hipStream_t)stream;
    if (B == 0 || P_r == 0) return neutral_state("pose_partials_fit", v, n, s);   // no kernel runs, tfit is empty
    if (!pred || !conn) return fail(PAFUSE_E_ARG, "pose_partials_fit: null pointer");
    unsigned grid;
    if (int rc = wave_grid("pose_partials_fit", (int64_t)B * T * F, grid)) return rc;   // one wave per (b, t, f)
    PoseFitParams m{};
    m.pred = pred, m.x2d = x2d, m.conf = conf, m.cam = cam, m.conn = conn, m.st = v, m.tfit = tfit;
    m.B = B, m.T = T, m.P = P_r, m.F = F, m.J = J, m.h0 = h0;
    return launch<pose_fit_partials_kernel>("pose_fit_partials_kernel", grid, 256, 0, s, m);
}

int pafuse_pose_combine(const void* states, int32_t W, size_t stride_bytes, int32_t B, int32_t T, int32_t F, int32_t J,
                        int32_t P_total, void* merged, float* mean, float* pick, int32_t* pick_idx, void* stream) {
    StreamDevice on_stream_device(stream);
    if (B < 0 || T <= 0 || F <= 0 || J <= 0 || W < 1) return fail(PAFUSE_E_ARG, "pose_combine: bad size");
    if (!merged && !mean && !pick && !pick_idx) return fail(PAFUSE_E_ARG, "pose_combine: nothing to write");
    if (mean && P_total < 1) return fail(PAFUSE_E_ARG, "pose_combine: P_total %d", P_total);
    const int64_t n = (int64_t)B * T * F * J;
    if (n == 0) return PAFUSE_OK;
    if (!states) return fail(PAFUSE_E_ARG, "pose_combine: null pointer");
    if (int rc = check_combine("pose_combine", states, W, stride_bytes, PoseStateViews::head_bytes(n), merged, MergeOver::First,
                               (n + 255) / 256)) return rc;
    PoseCombineParams c{};
    c.states = (const char*)states, c.stride = (int64_t)stride_bytes, c.W = W;
    if (merged) c.merged = PoseStateViews(merged, n);
    c.mean = mean, c.pick = pick, c.pick_idx = pick_idx, c.n = n, c.P = P_total;
    return launch<pose_combine_kernel>("pose_combine_kernel", blocks_for(n), 256, 0, (hipStream_t)stream, c);
}

// workspace of pafuse_pose_path: one back-pointer byte per (line, frame, hypothesis), rounded up to 8 bytes
size_t pafuse_pose_path_workspace_bytes(int32_t B, int32_t T, int32_t P, int32_t F, int32_t J) {
    if (B < 0 || T <= 0 || P <= 0 || F <= 0 || J <= 0) return 0;
    return ((size_t)B * T * J * F * P + 7) / 8 * 8;
}

// J-Agg coherent in time (pose_path_kernel): one wave per line (b, t, j); the argument checks come before the first HIP call
int pafuse_pose_path(const float* pred, const float* x2d, const float* root, int32_t root_per_hypothesis, const float* cam,
                     const float* conf, const int32_t* conn, const float* mean, double weight, int32_t B, int32_t T, int32_t P,
                     int32_t F, int32_t J, float* pick, int32_t* pick_idx, float* pick_e2, double* cost, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (B < 0 || T <= 0 || P <= 0 || F <= 0 || J <= 0) return fail(PAFUSE_E_ARG, "pose_path: bad size");
    if (!std::isfinite(weight) || weight < 0.0) return fail(PAFUSE_E_ARG, "pose_path: weight %g is not finite and >= 0", weight);
    if (P > 256 || F > 256) return fail(PAFUSE_E_SHAPE, "pose_path: P = %d, F = %d: at most 256 hypotheses and 256 frames", P, F);
    if (B == 0) return PAFUSE_OK;   // nothing to launch
    if (!pred || !x2d || !root || !cam || !conn || !pick || !pick_idx)
        return fail(PAFUSE_E_ARG, "pose_path: pred, x2d, root, cam, conn, pick and pick_idx are needed (conf, mean, pick_e2, cost may be null)");
    const size_t need = pafuse_pose_path_workspace_bytes(B, T, P, F, J);
    if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 8)
        return fail(PAFUSE_E_ARG, "pose_path: the workspace needs %zu bytes, 8-byte aligned", need);
    if ((uintptr_t)cost % 8) return fail(PAFUSE_E_ARG, "pose_path: cost must be 8-byte aligned");
    unsigned grid;
    if (int rc = wave_grid("pose_path", (int64_t)B * T * J, grid)) return rc;   // one wave per (b, t, j)
    StreamDevice on_stream_device(stream);
    PathParams m{};   // B clips: one window [0, F) each, no tables, no pick_win; slot = hypothesis
    m.pred = pred, m.x2d = x2d, m.root = root, m.cam = cam, m.conf = conf, m.conn = conn, m.mean = mean, m.weight = weight;
    m.pick = pick, m.pick_idx = pick_idx, m.pick_e2 = pick_e2, m.cost = cost, m.back = (uint8_t*)workspace;
    m.V = B, m.W = 1, m.T = T, m.P = P, m.F = F, m.J = J, m.N = F, m.K = P, m.root_per_h = root_per_hypothesis ? 1 : 0;
    return by_lane_slots(P, [&](auto r) { return launch<pose_path_kernel<decltype(r)::value>>("pose_path_kernel", grid, 256, 0, (hipStream_t)stream, m); });
}

namespace {
// What pafuse_frames_path asks of the window table of a video (the HOST copy): starts strictly ascending from 0, ends
// starts[w] + valid[w] not descending and ending at N, no gap, valid >= 1 (and <= F where F > 0).  -> nullptr and the largest
// number of windows that cover one frame, or what is wrong.  The windows that cover a frame are then a contiguous range,
// and the coverage peaks at some window's first frame.
const char* video_windows(const int32_t* starts, const int32_t* valid, int32_t W, int32_t F, int32_t N, int* cover) {
    if (W < 1 || N < 1) return "a video has at least one window and one frame";
    if (starts[0] != 0) return "the first window must start at frame 0";
    int lo = 0, most = 0;
    for (int w = 0; w < W; ++w) {
        if (valid[w] < 1 || (F > 0 && valid[w] > F)) return "valid must lie in 1 .. F";
        if (starts[w] < 0 || (int64_t)starts[w] + valid[w] > N) return "a window reaches past the N frames";
        if (w) {
            if (starts[w] <= starts[w - 1]) return "starts must ascend strictly";
            if (starts[w] + valid[w] < starts[w - 1] + valid[w - 1]) return "the windows' ends must not descend";
            if (starts[w] > starts[w - 1] + valid[w - 1]) return "a gap between two windows";
        }
        while (starts[lo] + valid[lo] <= starts[w]) ++lo;   // (lo <= w: window w covers its own first frame)
        most = w - lo + 1 > most ? w - lo + 1 : most;
    }
    if (starts[W - 1] + valid[W - 1] != N) return "the last window must end at frame N";
    *cover = most;
    return nullptr;
}
}  // namespace

// workspace of pafuse_frames_path: one back-pointer byte per (line, frame, slot), K = P * the largest coverage slots per
// frame, rounded up to 8 bytes; 0 for whatever the call would refuse
size_t pafuse_frames_path_workspace_bytes(int32_t N, int32_t T, int32_t J, int32_t P, int32_t W, const int32_t* starts_host,
                                          const int32_t* valid_host) {
    int cover = 0;
    if (N <= 0 || T <= 0 || J <= 0 || P <= 0 || W <= 0 || !starts_host || !valid_host) return 0;
    if (video_windows(starts_host, valid_host, W, 0, N, &cover) || (int64_t)cover * P > 256) return 0;
    return ((size_t)T * J * N * cover * P + 7) / 8 * 8;
}

// The path of a whole video (frames_path_kernel): one wave per line (t, j); the argument checks come before the first HIP call
int pafuse_frames_path(const float* pred, const float* x2d, const float* root, int32_t root_per_hypothesis, const float* cam,
                       const float* conf, const int32_t* conn, const float* mean, double weight, int32_t W, int32_t T, int32_t P,
                       int32_t F, int32_t J, int32_t N, const int32_t* starts, const int32_t* valid, const int32_t* starts_host,
                       const int32_t* valid_host, float* pick, int32_t* pick_idx, int32_t* pick_win, float* pick_e2, double* cost,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (W <= 0 || T <= 0 || P <= 0 || F <= 0 || J <= 0 || N <= 0)
        return fail(PAFUSE_E_ARG, "frames_path: bad size (a video has at least one window and one frame)");
    if (!std::isfinite(weight) || weight < 0.0) return fail(PAFUSE_E_ARG, "frames_path: weight %g is not finite and >= 0", weight);
    if (!pred || !x2d || !root || !cam || !conn || !starts || !valid || !starts_host || !valid_host || !pick || !pick_idx || !pick_win)
        return fail(PAFUSE_E_ARG, "frames_path: pred, x2d, root, cam, conn, the window tables (device and host), pick, pick_idx and "
                                  "pick_win are needed (conf, mean, pick_e2, cost may be null)");
    int cover = 0;
    if (const char* why = video_windows(starts_host, valid_host, W, F, N, &cover))
        return fail(PAFUSE_E_ARG, "frames_path: the windows must be the whole video of N = %d frames: %s", N, why);
    if ((int64_t)cover * P > 256)
        return fail(PAFUSE_E_SHAPE, "frames_path: %d windows cover one frame with P = %d hypotheses each: at most 256 candidates per frame", cover, P);
    const int K = cover * P;
    const size_t need = ((size_t)T * J * N * K + 7) / 8 * 8;
    if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 8)
        return fail(PAFUSE_E_ARG, "frames_path: the workspace needs %zu bytes, 8-byte aligned", need);
    if ((uintptr_t)cost % 8) return fail(PAFUSE_E_ARG, "frames_path: cost must be 8-byte aligned");
    unsigned grid;
    if (int rc = wave_grid("frames_path", (int64_t)T * J, grid)) return rc;   // one wave per (t, j)
    StreamDevice on_stream_device(stream);
    PathParams m{};   // one video
    m.pred = pred, m.x2d = x2d, m.root = root, m.cam = cam, m.conf = conf, m.conn = conn, m.mean = mean, m.weight = weight;
    m.starts = starts, m.valid = valid;
    m.pick = pick, m.pick_idx = pick_idx, m.pick_win = pick_win, m.pick_e2 = pick_e2, m.cost = cost, m.back = (uint8_t*)workspace;
    m.V = 1, m.W = W, m.T = T, m.P = P, m.F = F, m.J = J, m.N = N, m.K = K, m.root_per_h = root_per_hypothesis ? 1 : 0;
    return by_lane_slots(K, [&](auto r) { return launch<frames_path_kernel<decltype(r)::value>>("frames_path_kernel", grid, 256, 0, (hipStream_t)stream, m); });
}

// state of pafuse_spread_partials: double sum[n][3] | double m2[n][6] | double count
size_t pafuse_spread_partials_bytes(int32_t B, int32_t T, int32_t F, int32_t J) {
    if (B <= 0 || T <= 0 || F <= 0 || J <= 0) return 0;
    return ((size_t)B * T * F * J * 9 + 1) * 8;
}

int pafuse_spread_partials(const float* pred, const int32_t* conn, int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J,
                           int32_t h0, void* state, size_t state_bytes, void* stream) {
    StreamDevice on_stream_device(stream);
    if (B < 0 || T <= 0 || P_r < 0 || F <= 0 || J <= 0 || h0 < 0) return fail(PAFUSE_E_ARG, "spread_partials: bad size");
    const size_t need = pafuse_spread_partials_bytes(B, T, F, J);
    if (int rc = check_state("spread_partials", state, state_bytes, need)) return rc;
    const int64_t n = (int64_t)B * T * F * J;
    if (n == 0) return PAFUSE_OK;
    hipStream_t s = (hipStream_t)stream;
    if (P_r == 0) {   // the neutral state: zero sums, zero moments, count 0; no kernel runs
        hipError_t e = hipMemsetAsync(state, 0, need, s);
        if (e != hipSuccess) return fail(PAFUSE_E_HIP, "spread_partials: %s", hipGetErrorString(e));
        return PAFUSE_OK;
    }
    if (!pred || !conn) return fail(PAFUSE_E_ARG, "spread_partials: null pointer");
    if ((n + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "spread_partials: grid out of range");
    SpreadPartialsParams m{};
    m.pred = pred, m.conn = conn;
    m.sum = (double*)state, m.m2 = m.sum + 3 * n, m.count = m.sum + 9 * n;
    m.B = B, m.T = T, m.P = P_r, m.F = F, m.J = J;
    return launch<spread_partials_kernel>("spread_partials_kernel", blocks_for(n), 256, 0, s, m);
}

int pafuse_spread_combine(const void* states, int32_t W, size_t stride_bytes, int32_t B, int32_t T, int32_t F, int32_t J,
                          void* merged, float* mean, float* cov, float* std_dev, void* stream) {
    StreamDevice on_stream_device(stream);
    if (B < 0 || T <= 0 || F <= 0 || J <= 0 || W < 1) return fail(PAFUSE_E_ARG, "spread_combine: bad size");
    if (!merged && !mean && !cov && !std_dev) return fail(PAFUSE_E_ARG, "spread_combine: nothing to write");
    const int64_t n = (int64_t)B * T * F * J;
    if (n == 0) return PAFUSE_OK;
    if (!states) return fail(PAFUSE_E_ARG, "spread_combine: null pointer");
    const size_t need = pafuse_spread_partials_bytes(B, T, F, J);
    if (int rc = check_combine("spread_combine", states, W, stride_bytes, need, merged, MergeOver::First, (n + 255) / 256)) return rc;
    const char* lo = (const char*)states;
    SpreadCombineParams c{};
    c.states = lo, c.stride = (int64_t)stride_bytes, c.W = W, c.merged = (double*)merged;
    c.mean = mean, c.cov = cov, c.sd = std_dev, c.n = n;
    if (int rc = launch<spread_combine_kernel>("spread_combine_kernel", blocks_for(n), 256, 0, (hipStream_t)stream, c)) return rc;
    if (!merged) return PAFUSE_OK;
    // the merged count, behind the kernel whose every thread reads the operands' counts (the merged state may lie over the first)
    return launch<spread_count_kernel>("spread_count_kernel", 1, 64, 0, (hipStream_t)stream, lo, (int64_t)stride_bytes, W, n, (double*)merged);
}

// frame pose state: double sum[r][3] | float e2[r] | int32 idx[r] | int32 win[r] | float sel[r][3] | int32 count[N], r = T*N*J
size_t pafuse_frame_pose_state_bytes(int32_t N, int32_t T, int32_t J) {
    if (N <= 0 || T <= 0 || J <= 0) return 0;
    return FramePoseViews::bytes((int64_t)N * T * J, N);
}

// frame spread state: double sum[r][3] | double m2[r][6] | double count[N]
size_t pafuse_frame_spread_state_bytes(int32_t N, int32_t T, int32_t J) {
    if (N <= 0 || T <= 0 || J <= 0) return 0;
    return ((size_t)N * T * J * 9 + (size_t)N) * 8;
}

namespace {
// what both folds check of their window tables (the HOST copies) before anything is launched; -> the frame range touched
int check_windows(const char* who, const int32_t* starts, const int32_t* valid, int32_t B, int32_t F, int32_t N, int* n_lo, int* n_hi) {
    int hi = 0;
    for (int b = 0; b < B; ++b) {
        if (valid[b] < 1 || valid[b] > F) return fail(PAFUSE_E_ARG, "%s: valid[%d] = %d outside 1 .. %d", who, b, valid[b], F);
        if (starts[b] < 0 || (int64_t)starts[b] + valid[b] > N)
            return fail(PAFUSE_E_ARG, "%s: window %d covers frames [%d, %lld) of %d", who, b, starts[b], (long long)starts[b] + valid[b], N);
        if (b && starts[b] <= starts[b - 1]) return fail(PAFUSE_E_ARG, "%s: starts must ascend strictly (window %d)", who, b);
        hi = starts[b] + valid[b] > hi ? starts[b] + valid[b] : hi;
    }
    *n_lo = starts[0], *n_hi = hi;
    return PAFUSE_OK;
}
}  // namespace

int pafuse_frame_pose_state_init(void* frame_state, size_t frame_bytes, int32_t N, int32_t T, int32_t J, void* stream) {
    StreamDevice on_stream_device(stream);
    if (N < 0 || T <= 0 || J <= 0) return fail(PAFUSE_E_ARG, "frame_pose_state_init: bad size");
    const size_t need = pafuse_frame_pose_state_bytes(N, T, J);
    if (need == 0) return PAFUSE_OK;
    if (int rc = check_state("frame_pose_state_init", frame_state, frame_bytes, need)) return rc;
    const int64_t rows = (int64_t)N * T * J;
    FramePoseViews v(frame_state, rows);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = neutral_state("frame_pose_state_init", v, rows, s)) return rc;
    hipError_t e = hipMemsetAsync(v.win, 0xff, (size_t)rows * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(v.count, 0, (size_t)N * 4, s);
    if (e != hipSuccess) return fail(PAFUSE_E_HIP, "frame_pose_state_init: %s", hipGetErrorString(e));
    return PAFUSE_OK;
}

int pafuse_frame_spread_state_init(void* frame_state, size_t frame_bytes, int32_t N, int32_t T, int32_t J, void* stream) {
    StreamDevice on_stream_device(stream);
    if (N < 0 || T <= 0 || J <= 0) return fail(PAFUSE_E_ARG, "frame_spread_state_init: bad size");
    const size_t need = pafuse_frame_spread_state_bytes(N, T, J);
    if (need == 0) return PAFUSE_OK;
    if (int rc = check_state("frame_spread_state_init", frame_state, frame_bytes, need)) return rc;
    hipError_t e = hipMemsetAsync(frame_state, 0, need, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PAFUSE_E_HIP, "frame_spread_state_init: %s", hipGetErrorString(e));
    return PAFUSE_OK;
}

int pafuse_pose_windows_fold(void* frame_state, size_t frame_bytes, int32_t N, const void* state, size_t state_bytes, int32_t B,
                             int32_t T, int32_t F, int32_t J, const int32_t* starts, const int32_t* valid,
                             const int32_t* starts_host, const int32_t* valid_host, int32_t w0, int32_t P_total, void* stream) {
    StreamDevice on_stream_device(stream);
    if (N <= 0 || B < 0 || T <= 0 || F <= 0 || J <= 0 || w0 < 0 || P_total < 0) return fail(PAFUSE_E_ARG, "pose_windows_fold: bad size");
    const size_t fneed = pafuse_frame_pose_state_bytes(N, T, J);
    if (!frame_state || frame_bytes < fneed) return fail(PAFUSE_E_ARG, "pose_windows_fold: the frame state needs %zu bytes", fneed);
    if (B == 0) return PAFUSE_OK;   // nothing to fold, nothing is launched
    if (!state || !starts || !valid || !starts_host || !valid_host) return fail(PAFUSE_E_ARG, "pose_windows_fold: null pointer");
    const size_t need = pafuse_pose_partials_bytes(B, T, F, J);
    if (state_bytes < need) return fail(PAFUSE_E_ARG, "pose_windows_fold: the batch state needs %zu bytes", need);
    if ((uintptr_t)frame_state % 8 || (uintptr_t)state % 8) return fail(PAFUSE_E_ARG, "pose_windows_fold: states must be 8-byte aligned");
    int n_lo = 0, n_hi = 0;
    if (int rc = check_windows("pose_windows_fold", starts_host, valid_host, B, F, N, &n_lo, &n_hi)) return rc;
    const int64_t rows = (int64_t)N * T * J, sn = (int64_t)B * T * F * J, work = (int64_t)T * (n_hi - n_lo) * J;
    if ((work + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "pose_windows_fold: grid out of range");
    PoseWindowsFoldParams m{};
    m.frame = FramePoseViews(frame_state, rows), m.state = PoseStateViews(state, sn);
    m.starts = starts, m.valid = valid;
    m.N = N, m.B = B, m.T = T, m.F = F, m.J = J, m.w0 = w0, m.P = P_total, m.n_lo = n_lo, m.n_hi = n_hi;
    return launch<pose_windows_fold_kernel>("pose_windows_fold_kernel", blocks_for(work), 256, 0, (hipStream_t)stream, m);
}

int pafuse_spread_windows_fold(void* frame_state, size_t frame_bytes, int32_t N, const void* state, size_t state_bytes, int32_t B,
                               int32_t T, int32_t F, int32_t J, const int32_t* starts, const int32_t* valid,
                               const int32_t* starts_host, const int32_t* valid_host, void* stream) {
    StreamDevice on_stream_device(stream);
    if (N <= 0 || B < 0 || T <= 0 || F <= 0 || J <= 0) return fail(PAFUSE_E_ARG, "spread_windows_fold: bad size");
    const size_t fneed = pafuse_frame_spread_state_bytes(N, T, J);
    if (!frame_state || frame_bytes < fneed) return fail(PAFUSE_E_ARG, "spread_windows_fold: the frame state needs %zu bytes", fneed);
    if (B == 0) return PAFUSE_OK;   // nothing to fold, nothing is launched
    if (!state || !starts || !valid || !starts_host || !valid_host) return fail(PAFUSE_E_ARG, "spread_windows_fold: null pointer");
    const size_t need = pafuse_spread_partials_bytes(B, T, F, J);
    if (state_bytes < need) return fail(PAFUSE_E_ARG, "spread_windows_fold: the batch state needs %zu bytes", need);
    if ((uintptr_t)frame_state % 8 || (uintptr_t)state % 8) return fail(PAFUSE_E_ARG, "spread_windows_fold: states must be 8-byte aligned");
    int n_lo = 0, n_hi = 0;
    if (int rc = check_windows("spread_windows_fold", starts_host, valid_host, B, F, N, &n_lo, &n_hi)) return rc;
    const int64_t work = (int64_t)T * (n_hi - n_lo) * J;
    if ((work + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "spread_windows_fold: grid out of range");
    SpreadWindowsFoldParams m{};
    m.frame = (double*)frame_state, m.state = (const double*)state, m.starts = starts, m.valid = valid;
    m.N = N, m.B = B, m.T = T, m.F = F, m.J = J, m.n_lo = n_lo, m.n_hi = n_hi;
    if (int rc = launch<spread_windows_fold_kernel>("spread_windows_fold_kernel", blocks_for(work), 256, 0, (hipStream_t)stream, m)) return rc;
    // the counts, behind the kernel whose every thread reads them
    return launch<spread_windows_count_kernel>("spread_windows_count_kernel", blocks_for(n_hi - n_lo), 256, 0, (hipStream_t)stream, m);
}

int pafuse_frames_finish(const void* frame_state, const void* frame_spread, int32_t N, int32_t T, int32_t J, float* mean,
                         float* pick, int32_t* pick_idx, int32_t* pick_win, float* std_dev, float* cov, void* stream) {
    StreamDevice on_stream_device(stream);
    if (N < 0 || T <= 0 || J <= 0) return fail(PAFUSE_E_ARG, "frames_finish: bad size");
    const bool pose = mean || pick || pick_idx || pick_win, spread = std_dev || cov;
    if (!pose && !spread) return fail(PAFUSE_E_ARG, "frames_finish: nothing to write");
    if (N == 0) return PAFUSE_OK;
    if ((pose && !frame_state) || (spread && !frame_spread)) return fail(PAFUSE_E_ARG, "frames_finish: null pointer");
    if ((uintptr_t)frame_state % 8 || (uintptr_t)frame_spread % 8) return fail(PAFUSE_E_ARG, "frames_finish: states must be 8-byte aligned");
    const int64_t rows = (int64_t)N * T * J;
    if ((rows + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "frames_finish: grid out of range");
    FramesFinishParams m{};
    if (pose) m.frame = FramePoseViews(frame_state, rows);
    m.spread = spread ? (const double*)frame_spread : nullptr;
    m.mean = mean, m.pick = pick, m.pick_idx = pick_idx, m.pick_win = pick_win, m.sd = std_dev, m.cov = cov;
    m.N = N, m.T = T, m.J = J;
    return launch<frames_finish_kernel>("frames_finish_kernel", blocks_for(rows), 256, 0, (hipStream_t)stream, m);
}

// the camera-space root of every (t, frame) of the finished pose (frames_root_fit_kernel): the argument checks come before
// the first HIP call
int pafuse_frames_root_fit(const float* pose, const float* x2d, const float* conf, const float* cam, int32_t T, int32_t N,
                           int32_t J, float* traj, float* wsum, float* resid, void* stream) {
    if (!pose || !x2d || !cam || !traj) return fail(PAFUSE_E_ARG, "frames_root_fit: pose, x2d, cam and traj are needed (conf, wsum, resid may be null)");
    if (T < 1 || N < 1 || J < 1) return fail(PAFUSE_E_ARG, "frames_root_fit: bad size (T=%d N=%d J=%d)", T, N, J);
    unsigned grid;
    if (int rc = wave_grid("frames_root_fit", (int64_t)T * N, grid)) return rc;   // one wave per (t, n)
    StreamDevice on_stream_device(stream);
    FramesRootFitParams m{};
    m.pose = pose, m.x2d = x2d, m.conf = conf, m.cam = cam, m.traj = traj, m.wsum = wsum, m.resid = resid;
    m.T = T, m.N = N, m.J = J;
    return by_joint_slots(J, [&](auto slots) { return launch<frames_root_fit_kernel<decltype(slots)::value>>("frames_root_fit_kernel", grid, 256, 0, (hipStream_t)stream, m); });
}

// the confidence-weighted local-linear filter along the frames (trajectory_smooth_kernel)
int pafuse_trajectory_smooth(const float* traj, const float* weight, int32_t T, int32_t N, int32_t radius, float* out,
                             void* stream) {
    if (!traj || !out) return fail(PAFUSE_E_ARG, "trajectory_smooth: traj and out are needed (weight may be null: every weight 1)");
    if (T < 1 || N < 1) return fail(PAFUSE_E_ARG, "trajectory_smooth: bad size (T=%d N=%d)", T, N);
    if (radius < 1 || radius > 64) return fail(PAFUSE_E_ARG, "trajectory_smooth: radius %d outside 1 .. 64", radius);
    if (out == traj) return fail(PAFUSE_E_ARG, "trajectory_smooth: out may not alias traj (every thread reads its neighbours' frames)");
    const int64_t rows = (int64_t)T * N;
    if ((rows + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "trajectory_smooth: grid out of range");
    StreamDevice on_stream_device(stream);
    TrajectorySmoothParams m{};
    m.traj = traj, m.weight = weight, m.out = out, m.T = T, m.N = N, m.radius = radius;
    return launch<trajectory_smooth_kernel>("trajectory_smooth_kernel", blocks_for(rows), 256, 0, (hipStream_t)stream, m);
}

// missing 2-D detections filled along the frames, per joint (detections_repair_kernel): level 0, then - with a table - level 1
// on the same stream; the argument checks come before the first HIP call
int pafuse_detections_repair(const float* x2d, const float* conf, const int32_t* anchor, int32_t N, int32_t J, int32_t radius,
                             float threshold, float* out, float* conf_out, uint8_t* status, void* stream) {
    if (!x2d || !conf || !out || !status) return fail(PAFUSE_E_ARG, "detections_repair: x2d, conf, out and status are needed (anchor, conf_out may be null)");
    if (N < 1 || J < 1) return fail(PAFUSE_E_ARG, "detections_repair: bad size (N=%d J=%d)", N, J);
    if (radius < 1 || radius > 64) return fail(PAFUSE_E_ARG, "detections_repair: radius %d outside 1 .. 64", radius);
    if (!std::isfinite(threshold) || threshold < 0.f) return fail(PAFUSE_E_ARG, "detections_repair: threshold %g is not finite and >= 0", (double)threshold);
    if (out == x2d) return fail(PAFUSE_E_ARG, "detections_repair: out may not alias x2d (every thread reads its neighbours' frames)");
    if (conf_out && conf_out == conf) return fail(PAFUSE_E_ARG, "detections_repair: conf_out may not alias conf (the walk reads the confidences)");
    const int64_t rows = (int64_t)N * J;
    if ((rows + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "detections_repair: grid out of range");
    StreamDevice on_stream_device(stream);
    DetectionsRepairParams m{};
    m.x2d = x2d, m.conf = conf, m.anchor = anchor, m.out = out, m.conf_out = conf_out, m.status = status;
    m.N = N, m.J = J, m.radius = radius, m.threshold = threshold;
    for (int level = 0; level < (anchor ? 2 : 1); ++level) {
        m.level = level;
        const int rc = launch<detections_repair_kernel>("detections_repair_kernel", blocks_for(rows), 256, 0, (hipStream_t)stream, m);
        if (rc != PAFUSE_OK) return rc;
    }
    return PAFUSE_OK;
}

// observed 2-D detections screened in front of the repair (detections_residual_kernel, detections_scale_kernel,
// detections_screen_finish_kernel): pass 1's residuals, the scales, passes 2 .. K each gating its own residual, the evaluation
// against acc_K, the finish - passes + 3 launches on the stream; the argument checks come before the first HIP call.
// Workspace: tau [J] fp64, then e_1, e_self, e_cross [N,J] fp32, then the two acc buffers [N,J] bytes.
size_t pafuse_detections_screen_workspace_bytes(int32_t N, int32_t J) {
    return N < 1 || J < 1 ? 0 : (size_t)J * sizeof(double) + (size_t)N * (size_t)J * (3 * sizeof(float) + 2);
}

int pafuse_detections_screen(const float* x2d, const float* conf, const int32_t* mirror, int32_t N, int32_t J, int32_t radius,
                             int32_t passes, int32_t support, float threshold, float gate, float floor, float* out, float* conf_out,
                             uint8_t* status, float* resid, float* scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x2d || !conf || !out || !conf_out || !status)
        return fail(PAFUSE_E_ARG, "detections_screen: x2d, conf, out, conf_out and status are needed (mirror, resid, scale may be null)");
    if (N < 1 || J < 1) return fail(PAFUSE_E_ARG, "detections_screen: bad size (N=%d J=%d)", N, J);
    if (radius < 1 || radius > 64) return fail(PAFUSE_E_ARG, "detections_screen: radius %d outside 1 .. 64", radius);
    if (passes < 1 || passes > 8) return fail(PAFUSE_E_ARG, "detections_screen: passes %d outside 1 .. 8", passes);
    if (support < 2 || support > 129) return fail(PAFUSE_E_ARG, "detections_screen: support %d outside 2 .. 129", support);
    if (!std::isfinite(threshold) || threshold < 0.f) return fail(PAFUSE_E_ARG, "detections_screen: threshold %g is not finite and >= 0", (double)threshold);
    if (!std::isfinite(gate) || !(gate > 0.f)) return fail(PAFUSE_E_ARG, "detections_screen: gate %g is not finite and > 0", (double)gate);
    if (!std::isfinite(floor) || !(floor > 0.f)) return fail(PAFUSE_E_ARG, "detections_screen: floor %g is not finite and > 0", (double)floor);
    if (out == x2d) return fail(PAFUSE_E_ARG, "detections_screen: out may not alias x2d (every launch reads the input)");
    if (conf_out == conf) return fail(PAFUSE_E_ARG, "detections_screen: conf_out may not alias conf (every launch reads the confidences)");
    const int64_t rows = (int64_t)N * J;      // the grid first: within it the workspace size cannot overflow
    if ((rows + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "detections_screen: grid out of range");
    const size_t need = pafuse_detections_screen_workspace_bytes(N, J);
    if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 8)
        return fail(PAFUSE_E_ARG, "detections_screen: the workspace must hold %zu bytes, 8-byte aligned (pafuse_detections_screen_workspace_bytes)", need);
    unsigned waves;
    if (int rc = wave_grid("detections_screen", J, waves)) return rc;   // one wave per joint
    StreamDevice on_stream_device(stream);
    double* tau = (double*)workspace;
    float* e1 = (float*)(tau + J);
    float *e_self = e1 + rows, *e_cross = e_self + rows;
    uint8_t* acc[2] = {(uint8_t*)(e_cross + rows), (uint8_t*)(e_cross + rows) + rows};
    const unsigned grid = blocks_for(rows);
    const hipStream_t s = (hipStream_t)stream;
    DetectionsScreenParams m{};
    m.x2d = x2d, m.conf = conf, m.mirror = mirror, m.e1 = e1, m.tau = tau;
    m.N = N, m.J = J, m.radius = radius, m.support = support, m.threshold = threshold;
    m.source = SCREEN_OBSERVED, m.e = e1;                                  // pass 1: e_1 against acc_0
    if (int rc = launch<detections_residual_kernel>("detections_residual_kernel", grid, 256, 0, s, m)) return rc;
    DetectionsScaleParams sc{};
    sc.e1 = e1, sc.tau = tau, sc.scale = scale, sc.N = N, sc.J = J, sc.gate = gate, sc.floor = floor;
    if (int rc = launch<detections_scale_kernel>("detections_scale_kernel", waves, 256, 0, s, sc)) return rc;
    m.e = nullptr, m.source = SCREEN_FIRST;                                // acc_1 is formed from e_1 and tau where it is read
    for (int pass = 2; pass <= passes; ++pass) {                           // reads acc_{pass-1}, writes acc_pass
        m.acc_next = acc[pass & 1];
        if (int rc = launch<detections_residual_kernel>("detections_residual_kernel", grid, 256, 0, s, m)) return rc;
        m.source = SCREEN_STORED, m.acc = m.acc_next;
    }
    m.acc_next = nullptr, m.e = e_self, m.e_cross = mirror ? e_cross : nullptr;   // against acc_K
    if (int rc = launch<detections_residual_kernel>("detections_residual_kernel", grid, 256, 0, s, m)) return rc;
    m.e = nullptr, m.e_cross = nullptr;
    m.e_self = e_self, m.e_cross_in = mirror ? e_cross : nullptr;
    m.out = out, m.conf_out = conf_out, m.status = status, m.resid = resid;
    return launch<detections_screen_finish_kernel>("detections_screen_finish_kernel", grid, 256, 0, s, m);
}

// people followed through a video (track_nodes_kernel, track_links_kernel, track_path_kernel, track_gather_kernel); the
// argument checks come before the first HIP call.  Workspace: gain [N,G,K,K] fp64, size [N,K] fp64, the back-pointers
// [N,K,2] bytes, the used flags [N,K] bytes, rounded up to a multiple of 8; J takes no part in the size.
struct TracksViews {
    double *gain, *size;
    uint8_t *back, *used;
    TracksViews(void* ws, int64_t N, int64_t K, int64_t G) {
        gain = (double*)ws, size = gain + N * G * K * K;
        back = (uint8_t*)(size + N * K), used = back + 2 * N * K;
    }
};

size_t pafuse_tracks_workspace_bytes(int32_t N, int32_t K, int32_t J, int32_t G) {
    if (N < 1 || K < 1 || K > TRACK_MAX_K || J < 1 || G < 1 || G > TRACK_MAX_GAP) return 0;
    const size_t nodes = (size_t)N * (size_t)K;
    return (nodes * (size_t)G * (size_t)K * sizeof(double) + nodes * (sizeof(double) + 3) + 7) / 8 * 8;
}

static int tracks_sizes(const char* who, int32_t N, int32_t K, int32_t G, const void* workspace, size_t workspace_bytes) {
    if (N < 1) return fail(PAFUSE_E_ARG, "%s: bad size (N=%d)", who, N);
    if (K < 1 || K > TRACK_MAX_K) return fail(PAFUSE_E_ARG, "%s: K %d outside 1 .. %d (pass the largest number of people in any frame)", who, K, TRACK_MAX_K);
    if (G < 1 || G > TRACK_MAX_GAP) return fail(PAFUSE_E_ARG, "%s: max_gap %d outside 1 .. %d", who, G, TRACK_MAX_GAP);
    if (((int64_t)N * G * K + 3) / 4 > 0x7fffffff) return fail(PAFUSE_E_ARG, "%s: grid out of range", who);   // the grid first: within it no size overflows
    const size_t need = pafuse_tracks_workspace_bytes(N, K, 1, G);
    if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 8)
        return fail(PAFUSE_E_ARG, "%s: the workspace must hold %zu bytes, 8-byte aligned (pafuse_tracks_workspace_bytes)", who, need);
    return PAFUSE_OK;
}

int pafuse_tracks_links(const float* x2d, const float* conf, int32_t N, int32_t K, int32_t J, int32_t G, int32_t support,
                        float threshold, double gate, double skip, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x2d || !conf) return fail(PAFUSE_E_ARG, "tracks_links: x2d and conf are needed");
    if (J < 1) return fail(PAFUSE_E_ARG, "tracks_links: bad size (J=%d)", J);
    if (support < 1 || support > 65535) return fail(PAFUSE_E_ARG, "tracks_links: support %d outside 1 .. 65535", support);
    if (!std::isfinite(threshold) || threshold < 0.f) return fail(PAFUSE_E_ARG, "tracks_links: threshold %g is not finite and >= 0", (double)threshold);
    if (!std::isfinite(gate) || !(gate > 0.0)) return fail(PAFUSE_E_ARG, "tracks_links: gate %g is not finite and > 0", gate);
    if (!std::isfinite(skip) || skip < 0.0) return fail(PAFUSE_E_ARG, "tracks_links: skip %g is not finite and >= 0", skip);
    if (int rc = tracks_sizes("tracks_links", N, K, G, workspace, workspace_bytes)) return rc;
    unsigned node_grid, link_grid;
    if (int rc = wave_grid("tracks_links", (int64_t)N * K, node_grid)) return rc;       // one wave per (n, k)
    if (int rc = wave_grid("tracks_links", (int64_t)N * G * K, link_grid)) return rc;   // one wave per (n, g, kb)
    StreamDevice on_stream_device(stream);
    const TracksViews v(workspace, N, K, G);
    TrackLinksParams m{};
    m.x2d = x2d, m.conf = conf, m.size = v.size, m.gain = v.gain, m.gate = gate, m.skip = skip, m.threshold = threshold;
    m.N = N, m.K = K, m.J = J, m.G = G, m.support = support;
    return by_joint_slots(J, [&](auto slots) {
        constexpr int S = decltype(slots)::value;
        if (int rc = launch<track_nodes_kernel<S>>("track_nodes_kernel", node_grid, 256, 0, (hipStream_t)stream, m)) return rc;
        return launch<track_links_kernel<S>>("track_links_kernel", link_grid, 256, 0, (hipStream_t)stream, m);
    });
}

int pafuse_tracks_path(const double* gain, const double* size, int32_t N, int32_t K, int32_t G, int32_t M, int32_t min_frames,
                       int32_t seed_n, int32_t seed_k, int32_t* assign, double* score, int32_t* frames, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (!assign || !score || !frames) return fail(PAFUSE_E_ARG, "tracks_path: assign, score and frames are needed (gain, size null: the workspace's own)");
    if (M < 1 || M > 64) return fail(PAFUSE_E_ARG, "tracks_path: tracks %d outside 1 .. 64", M);
    if (min_frames < 1) return fail(PAFUSE_E_ARG, "tracks_path: min_frames %d is not >= 1", min_frames);
    if (int rc = tracks_sizes("tracks_path", N, K, G, workspace, workspace_bytes)) return rc;
    const bool seeded = seed_n >= 0 || seed_k >= 0;
    if (seeded && !(seed_n >= 0 && seed_n < N && seed_k >= 0 && seed_k < K))
        return fail(PAFUSE_E_ARG, "tracks_path: seed (%d, %d) outside [0, %d) x [0, %d) (no seed: -1, -1)", seed_n, seed_k, N, K);
    if (seeded && M != 1) return fail(PAFUSE_E_ARG, "tracks_path: a seed names one person, it goes with tracks = 1 (got %d)", M);
    if ((uintptr_t)gain % 8 || (uintptr_t)size % 8) return fail(PAFUSE_E_ARG, "tracks_path: gain and size must be 8-byte aligned");
    StreamDevice on_stream_device(stream);
    const TracksViews v(workspace, N, K, G);
    TrackPathParams m{};
    m.gain = gain ? gain : v.gain, m.size = size ? size : v.size, m.assign = assign, m.score = score, m.frames = frames;
    m.back = v.back, m.used = v.used;
    m.N = N, m.K = K, m.G = G, m.M = M, m.min_frames = min_frames, m.seed_n = seeded ? seed_n : -1, m.seed_k = seeded ? seed_k : -1;
    return launch<track_path_kernel>("track_path_kernel", 1, 64, 0, (hipStream_t)stream, m);
}

int pafuse_tracks_gather(const float* x2d, const float* conf, const int32_t* assign, int32_t N, int32_t K, int32_t J, int32_t M,
                         float* out, float* conf_out, void* stream) {
    if (!x2d || !conf || !assign || !out || !conf_out) return fail(PAFUSE_E_ARG, "tracks_gather: x2d, conf, assign, out and conf_out are needed");
    if (N < 1 || J < 1) return fail(PAFUSE_E_ARG, "tracks_gather: bad size (N=%d J=%d)", N, J);
    if (K < 1 || K > TRACK_MAX_K) return fail(PAFUSE_E_ARG, "tracks_gather: K %d outside 1 .. %d", K, TRACK_MAX_K);
    if (M < 1 || M > 64) return fail(PAFUSE_E_ARG, "tracks_gather: tracks %d outside 1 .. 64", M);
    const int64_t rows = (int64_t)M * N * J;
    if ((rows + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "tracks_gather: grid out of range");
    StreamDevice on_stream_device(stream);
    TrackGatherParams m{};
    m.x2d = x2d, m.conf = conf, m.assign = assign, m.out = out, m.conf_out = conf_out, m.N = N, m.K = K, m.J = J, m.M = M;
    return launch<track_gather_kernel>("track_gather_kernel", blocks_for(rows), 256, 0, (hipStream_t)stream, m);
}

// the per-frame pose smoothed along the frames with the inverse hypothesis covariance as matrix weight (pose_precision_kernel,
// then pose_smooth_kernel, on the stream); the argument checks come before the first HIP call
size_t pafuse_pose_smooth_workspace_bytes(int32_t T, int32_t N, int32_t J) {
    return T < 1 || N < 1 || J < 1 ? 0 : (size_t)T * (size_t)N * (size_t)J * 6 * sizeof(double);
}

int pafuse_pose_smooth(const float* pose, const float* cov, int32_t T, int32_t N, int32_t J, int32_t radius, float floor,
                       float* out, uint8_t* code, void* workspace, size_t workspace_bytes, void* stream) {
    if (!pose || !out) return fail(PAFUSE_E_ARG, "pose_smooth: pose and out are needed (cov may be null: zeros; code may be null)");
    if (T < 1 || N < 1 || J < 1) return fail(PAFUSE_E_ARG, "pose_smooth: bad size (T=%d N=%d J=%d)", T, N, J);
    if (radius < 1 || radius > 64) return fail(PAFUSE_E_ARG, "pose_smooth: radius %d outside 1 .. 64", radius);
    if (!std::isfinite(floor) || !(floor > 0.f)) return fail(PAFUSE_E_ARG, "pose_smooth: floor %g is not finite and > 0", (double)floor);
    if (out == pose) return fail(PAFUSE_E_ARG, "pose_smooth: out may not alias pose (every thread reads its neighbours' frames)");
    const size_t need = pafuse_pose_smooth_workspace_bytes(T, N, J);
    if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 8)
        return fail(PAFUSE_E_ARG, "pose_smooth: the workspace must hold %zu bytes, 8-byte aligned (pafuse_pose_smooth_workspace_bytes)", need);
    const int64_t rows = (int64_t)T * N * J;
    if ((rows + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "pose_smooth: grid out of range");
    StreamDevice on_stream_device(stream);
    PoseSmoothParams m{};
    m.pose = pose, m.cov = cov, m.out = out, m.code = code, m.T = T, m.N = N, m.J = J, m.radius = radius, m.floor = floor;
    m.precision = (double*)workspace;
    const int rc = launch<pose_precision_kernel>("pose_precision_kernel", blocks_for(rows), 256, 0, (hipStream_t)stream, m);
    if (rc != PAFUSE_OK) return rc;
    return launch<pose_smooth_kernel>("pose_smooth_kernel", blocks_for(rows), 256, 0, (hipStream_t)stream, m);
}

// bone lengths held constant along a video: the weighted length of every bone (bone_lengths_kernel) and every frame projected
// onto the lengths of its step (bone_project_kernel); one kernel each, the argument checks come before the first HIP call
int pafuse_bone_lengths(const float* pose, const float* cov, const int32_t* parent, const int32_t* mirror, int32_t T, int32_t N,
                        int32_t J, float floor, float* length, float* dev, int32_t* frames, void* stream) {
    if (!pose || !parent || !length)
        return fail(PAFUSE_E_ARG, "bone_lengths: pose, parent and length are needed (cov, mirror, dev and frames may be null)");
    if (T < 1 || N < 1 || J < 1) return fail(PAFUSE_E_ARG, "bone_lengths: bad size (T=%d N=%d J=%d)", T, N, J);
    if (J > 256) return fail(PAFUSE_E_ARG, "bone_lengths: J = %d is more than 256", J);
    if (!std::isfinite(floor) || !(floor > 0.f)) return fail(PAFUSE_E_ARG, "bone_lengths: floor %g is not finite and > 0", (double)floor);
    unsigned grid;
    if (int rc = wave_grid("bone_lengths", (int64_t)T * J, grid)) return rc;   // one wave per (t, j)
    StreamDevice on_stream_device(stream);
    BoneLengthsParams m{};
    m.pose = pose, m.cov = cov, m.parent = parent, m.mirror = mirror, m.length = length, m.dev = dev, m.frames = frames;
    m.T = T, m.N = N, m.J = J, m.floor = floor;
    return launch<bone_lengths_kernel>("bone_lengths_kernel", grid, 256, 0, (hipStream_t)stream, m);
}

int pafuse_bone_project(const float* pose, const float* cov, const int32_t* parent, const float* length, int32_t T, int32_t N,
                        int32_t J, int32_t iterations, int32_t snap, float floor, float* out, uint8_t* code, float* resid,
                        void* stream) {
    if (!pose || !parent || !length || !out)
        return fail(PAFUSE_E_ARG, "bone_project: pose, parent, length and out are needed (cov, code and resid may be null)");
    if (T < 1 || N < 1 || J < 1) return fail(PAFUSE_E_ARG, "bone_project: bad size (T=%d N=%d J=%d)", T, N, J);
    if (J > 256) return fail(PAFUSE_E_ARG, "bone_project: J = %d is more than 256", J);
    if (iterations < 0 || iterations > 64) return fail(PAFUSE_E_ARG, "bone_project: iterations %d outside 0 .. 64", iterations);
    if (snap != 0 && snap != 1) return fail(PAFUSE_E_ARG, "bone_project: snap must be 0 or 1, got %d", snap);
    if (!std::isfinite(floor) || !(floor > 0.f)) return fail(PAFUSE_E_ARG, "bone_project: floor %g is not finite and > 0", (double)floor);
    if (out == pose) return fail(PAFUSE_E_ARG, "bone_project: out may not alias pose (a joint without an active bone keeps the input's bits)");
    unsigned grid;
    if (int rc = wave_grid("bone_project", (int64_t)T * N, grid)) return rc;   // one wave per (t, n)
    StreamDevice on_stream_device(stream);
    BoneProjectParams m{};
    m.pose = pose, m.cov = cov, m.parent = parent, m.length = length, m.out = out, m.code = code, m.resid = resid;
    m.T = T, m.N = N, m.J = J, m.iterations = iterations, m.snap = snap, m.floor = floor;
    return by_lane_slots(J, [&](auto r) { return launch<bone_project_kernel<decltype(r)::value>>("bone_project_kernel", grid, 256, 0, (hipStream_t)stream, m); });
}

// the focal-length sums of every (t, frame) of the finished pose (frames_focal_sums_kernel) and the estimate from them
// (focal_solve_kernel): the argument checks come before the first HIP call
int pafuse_frames_focal_sums(const float* pose, const float* x2d, const float* conf, const float* cam, int32_t T, int32_t N,
                             int32_t J, double* state, void* stream) {
    if (!pose || !x2d || !cam || !state) return fail(PAFUSE_E_ARG, "frames_focal_sums: pose, x2d, cam and state are needed (conf may be null)");
    if (T < 1 || N < 1 || J < 1) return fail(PAFUSE_E_ARG, "frames_focal_sums: bad size (T=%d N=%d J=%d)", T, N, J);
    if ((uintptr_t)state % 8) return fail(PAFUSE_E_ARG, "frames_focal_sums: state must be 8-byte aligned");
    unsigned grid;
    if (int rc = wave_grid("frames_focal_sums", (int64_t)T * N, grid)) return rc;   // one wave per (t, n)
    StreamDevice on_stream_device(stream);
    FramesFocalSumsParams m{};
    m.pose = pose, m.x2d = x2d, m.conf = conf, m.cam = cam, m.state = state;
    m.T = T, m.N = N, m.J = J;
    return by_joint_slots(J, [&](auto slots) { return launch<frames_focal_sums_kernel<decltype(slots)::value>>("frames_focal_sums_kernel", grid, 256, 0, (hipStream_t)stream, m); });
}

int pafuse_focal_solve(const double* state, int32_t T, int32_t N, const float* cam, int32_t cam_len, float* focal, float* r2,
                       int32_t* frames, float* cam_out, void* stream) {
    if (!state || !cam || !focal) return fail(PAFUSE_E_ARG, "focal_solve: state, cam and focal are needed (r2, frames, cam_out may be null)");
    if (T < 1 || N < 1) return fail(PAFUSE_E_ARG, "focal_solve: bad size (T=%d N=%d)", T, N);
    if (cam_len < 4 || cam_len > 9) return fail(PAFUSE_E_ARG, "focal_solve: cam_len %d outside 4 .. 9", cam_len);
    if ((uintptr_t)state % 8) return fail(PAFUSE_E_ARG, "focal_solve: state must be 8-byte aligned");
    unsigned grid;
    if (int rc = wave_grid("focal_solve", (int64_t)T, grid)) return rc;   // one wave per t
    StreamDevice on_stream_device(stream);
    FocalSolveParams m{};
    m.state = state, m.cam = cam, m.focal = focal, m.r2 = r2, m.frames = frames, m.cam_out = cam_out;
    m.T = T, m.N = N, m.cam_len = cam_len;
    return launch<focal_solve_kernel>("focal_solve_kernel", grid, 256, 0, (hipStream_t)stream, m);
}

// the ground plane of a video from its foot contacts and the poses in world space (foot_contacts_kernel, ground_sums_kernel,
// ground_solve_kernel, frames_to_world_kernel): one kernel each, the argument checks come before the first HIP call
static bool ground_positive(double v) { return std::isfinite(v) && v > 0.0; }

int pafuse_foot_contacts(const float* pose, const float* traj, const int32_t* points, int32_t T, int32_t N, int32_t J, int32_t K,
                         int32_t radius, double speed, float* foot, float* foot_speed, float* contact, void* stream) {
    if (!pose || !traj || !points || !foot || !contact)
        return fail(PAFUSE_E_ARG, "foot_contacts: pose, traj, points, foot and contact are needed (foot_speed may be null)");
    if (T < 1 || N < 1 || J < 1) return fail(PAFUSE_E_ARG, "foot_contacts: bad size (T=%d N=%d J=%d)", T, N, J);
    if (K < 1 || K > GROUND_MAX_POINTS) return fail(PAFUSE_E_ARG, "foot_contacts: K = %d outside 1 .. %d", K, GROUND_MAX_POINTS);
    if (radius < 1 || radius > 64) return fail(PAFUSE_E_ARG, "foot_contacts: radius %d outside 1 .. 64", radius);
    if (!ground_positive(speed)) return fail(PAFUSE_E_ARG, "foot_contacts: speed %g is not finite and > 0 (metres per frame)", speed);
    const int64_t rows = (int64_t)T * N * K;
    if ((rows + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "foot_contacts: grid out of range");
    StreamDevice on_stream_device(stream);
    FootContactsParams m{};
    m.pose = pose, m.traj = traj, m.points = points, m.foot = foot, m.foot_speed = foot_speed, m.contact = contact;
    m.speed = speed, m.T = T, m.N = N, m.J = J, m.K = K, m.radius = radius;
    return launch<foot_contacts_kernel>("foot_contacts_kernel", blocks_for(rows), 256, 0, (hipStream_t)stream, m);
}

int pafuse_ground_sums(const float* foot, const float* contact, const float* traj, const double* plane, const double* scale,
                       int32_t T, int32_t N, int32_t K, double gate, double* state, void* stream) {
    if (!foot || !contact || !traj || !state) return fail(PAFUSE_E_ARG, "ground_sums: foot, contact, traj and state are needed");
    if ((plane == nullptr) != (scale == nullptr)) return fail(PAFUSE_E_ARG, "ground_sums: plane and scale come together (or neither: the first pass)");
    if (T < 1 || N < 1) return fail(PAFUSE_E_ARG, "ground_sums: bad size (T=%d N=%d)", T, N);
    if (K < 1 || K > GROUND_MAX_POINTS) return fail(PAFUSE_E_ARG, "ground_sums: K = %d outside 1 .. %d", K, GROUND_MAX_POINTS);
    if (!ground_positive(gate)) return fail(PAFUSE_E_ARG, "ground_sums: gate %g is not finite and > 0", gate);
    if ((uintptr_t)state % 8 || (uintptr_t)plane % 8 || (uintptr_t)scale % 8)
        return fail(PAFUSE_E_ARG, "ground_sums: state, plane and scale must be 8-byte aligned");
    const int64_t rows = (int64_t)T * N;
    if ((rows + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "ground_sums: grid out of range");
    StreamDevice on_stream_device(stream);
    GroundSumsParams m{};
    m.foot = foot, m.contact = contact, m.traj = traj, m.plane = plane, m.scale = scale, m.state = state;
    m.gate = gate, m.T = T, m.N = N, m.K = K;
    return launch<ground_sums_kernel>("ground_sums_kernel", blocks_for(rows), 256, 0, (hipStream_t)stream, m);
}

int pafuse_ground_solve(const double* state, int32_t T, int32_t N, double floor, double spread, double* plane, double* scale,
                        float* up, float* camera_height, float* rms, float* eig, int32_t* points, uint8_t* code, void* stream) {
    if (!state || !plane || !scale)
        return fail(PAFUSE_E_ARG, "ground_solve: state, plane and scale are needed (up, camera_height, rms, eig, points, code may be null)");
    if (T < 1 || N < 1) return fail(PAFUSE_E_ARG, "ground_solve: bad size (T=%d N=%d)", T, N);
    if (!ground_positive(floor)) return fail(PAFUSE_E_ARG, "ground_solve: floor %g is not finite and > 0 (metres)", floor);
    if (!ground_positive(spread)) return fail(PAFUSE_E_ARG, "ground_solve: spread %g is not finite and > 0 (metres)", spread);
    if ((uintptr_t)state % 8 || (uintptr_t)plane % 8 || (uintptr_t)scale % 8)
        return fail(PAFUSE_E_ARG, "ground_solve: state, plane and scale must be 8-byte aligned");
    unsigned grid;
    if (int rc = wave_grid("ground_solve", (int64_t)T, grid)) return rc;   // one wave per t
    StreamDevice on_stream_device(stream);
    GroundSolveParams m{};
    m.state = state, m.plane = plane, m.scale = scale, m.up = up, m.height = camera_height, m.rms = rms, m.eig = eig;
    m.points = points, m.code = code, m.floor = floor, m.spread = spread, m.T = T, m.N = N;
    return launch<ground_solve_kernel>("ground_solve_kernel", grid, 256, 0, (hipStream_t)stream, m);
}

int pafuse_frames_to_world(const float* pose, const float* traj, const double* plane, int32_t T, int32_t N, int32_t J,
                           float* pose_world, float* traj_world, void* stream) {
    if (!pose || !traj || !plane || !pose_world)
        return fail(PAFUSE_E_ARG, "frames_to_world: pose, traj, plane and pose_world are needed (traj_world may be null)");
    if (T < 1 || N < 1 || J < 1) return fail(PAFUSE_E_ARG, "frames_to_world: bad size (T=%d N=%d J=%d)", T, N, J);
    if ((uintptr_t)plane % 8) return fail(PAFUSE_E_ARG, "frames_to_world: plane must be 8-byte aligned");
    const int64_t rows = (int64_t)T * N * J;
    if ((rows + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "frames_to_world: grid out of range");
    StreamDevice on_stream_device(stream);
    FramesToWorldParams m{};
    m.pose = pose, m.traj = traj, m.plane = plane, m.pose_world = pose_world, m.traj_world = traj_world;
    m.T = T, m.N = N, m.J = J;
    return launch<frames_to_world_kernel>("frames_to_world_kernel", blocks_for(rows), 256, 0, (hipStream_t)stream, m);
}

// the frame-level errors of the per-frame pose against ground truth (frame_errors_kernel) and their sums over the frames
// (frame_errors_reduce_kernel): the argument checks come before the first HIP call
static_assert(FRAME_MAX_PARTS == PAFUSE_MAX_PARTS, "frame_errors_kernel keeps one register slot per part");

int pafuse_frame_errors(const float* pose, const float* gt, const float* traj, const float* gt_root, const int32_t* pbroot,
                        const int32_t* part, int32_t num_parts, int32_t T, int32_t N, int32_t J, double* err, int32_t* cnt,
                        void* stream) {
    if (!pose || !gt || !pbroot || !part || !err || !cnt) return fail(PAFUSE_E_ARG, "frame_errors: pose, gt, pbroot, part, err and cnt are needed");
    if ((traj == nullptr) != (gt_root == nullptr)) return fail(PAFUSE_E_ARG, "frame_errors: traj and gt_root come together (or neither)");
    if (T < 1 || N < 1 || J < 1) return fail(PAFUSE_E_ARG, "frame_errors: bad size (T=%d N=%d J=%d)", T, N, J);
    if (num_parts < 1 || num_parts > PAFUSE_MAX_PARTS) return fail(PAFUSE_E_SHAPE, "frame_errors: num_parts %d outside 1 .. %d", num_parts, PAFUSE_MAX_PARTS);
    unsigned grid;
    if (int rc = wave_grid("frame_errors", (int64_t)T * N, grid)) return rc;   // one wave per (t, n)
    StreamDevice on_stream_device(stream);
    FrameErrorsParams m{};
    m.pose = pose, m.gt = gt, m.traj = traj, m.gt_root = gt_root, m.pbroot = pbroot, m.part = part, m.err = err, m.cnt = cnt;
    m.T = T, m.N = N, m.J = J, m.K = 6 + num_parts;
    return by_joint_slots(J, [&](auto slots) { return launch<frame_errors_kernel<decltype(slots)::value>>("frame_errors_kernel", grid, 256, 0, (hipStream_t)stream, m); });
}

int pafuse_frame_errors_reduce(const double* err, const int32_t* cnt, int32_t T, int32_t N, int32_t K, double* sums,
                               int64_t* counts, void* stream) {
    if (!err || !cnt || !sums || !counts) return fail(PAFUSE_E_ARG, "frame_errors_reduce: null pointer");
    if (T < 1 || N < 1) return fail(PAFUSE_E_ARG, "frame_errors_reduce: bad size (T=%d N=%d)", T, N);
    if (K < 7 || K > 6 + PAFUSE_MAX_PARTS) return fail(PAFUSE_E_SHAPE, "frame_errors_reduce: K = %d outside 7 .. %d (6 + num_parts)", K, 6 + PAFUSE_MAX_PARTS);
    unsigned grid;
    if (int rc = wave_grid("frame_errors_reduce", (int64_t)T * K, grid)) return rc;   // one wave per (t, k)
    StreamDevice on_stream_device(stream);
    FrameErrorsReduceParams m{};
    m.err = err, m.cnt = cnt, m.sums = sums, m.counts = counts, m.T = T, m.N = N, m.K = K;
    return launch<frame_errors_reduce_kernel>("frame_errors_reduce_kernel", grid, 256, 0, (hipStream_t)stream, m);
}

int pafuse_procrustes_errors(const float* pred, const float* gt, const float* x2d, const float* traj, const float* cam,
                             const int32_t* conn, int32_t B, int32_t T, int32_t P, int32_t F, int32_t J, float* jbest,
                             double* pbest_sums, float* pagg, float* jagg, int32_t* pick, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!pred || !gt || !x2d || !traj || !cam || !conn || !jbest || !pbest_sums || !pagg || !jagg)
        return fail(PAFUSE_E_ARG, "procrustes_errors: null pointer");
    if (B <= 0 || T <= 0 || P <= 0 || F <= 0 || J <= 0) return fail(PAFUSE_E_ARG, "procrustes_errors: bad size");
    if (J > P2_MAX_J) return fail(PAFUSE_E_ARG, "procrustes_errors: J = %d above the supported %d", J, P2_MAX_J);
    const int64_t n = (int64_t)B * T * F;
    if (n > 0x7fffffff) return fail(PAFUSE_E_ARG, "procrustes_errors: B*T*F = %lld workgroups", (long long)n);
    ProcrustesParams m{};
    m.pred = pred, m.gt = gt, m.x2d = x2d, m.traj = traj, m.cam = cam, m.conn = conn;
    m.jbest = jbest, m.pagg = pagg, m.jagg = jagg, m.pbest_sums = pbest_sums, m.pick = pick;
    m.B = B, m.T = T, m.P = P, m.F = F, m.J = J;
    return launch<procrustes_kernel>("procrustes_kernel", (unsigned)n, 64 * P2_WAVES, 0, (hipStream_t)stream, m);
}

// state of pafuse_procrustes_partials: float jbest[n], e2[n], sel[n] | int32 idx[n] | double psum[P_r][T]
static bool p2_partials_sizes_ok(int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J) {
    return B >= 0 && T > 0 && P_r >= 0 && F > 0 && J > 0;
}

size_t pafuse_procrustes_partials_bytes(int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J) {
    if (!p2_partials_sizes_ok(B, T, P_r, F, J)) return 0;
    return P2StateViews::head_bytes((int64_t)B * T * F * J) + (size_t)P_r * T * 8;
}

size_t pafuse_procrustes_partials_workspace_bytes(int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J) {
    if (!p2_partials_sizes_ok(B, T, P_r, F, J)) return 0;
    return (size_t)B * T * P_r * F * 8;
}

int pafuse_procrustes_partials(const float* pred, const float* gt, const float* x2d, const float* traj, const float* cam,
                               const int32_t* conn, int32_t B, int32_t T, int32_t P_r, int32_t F, int32_t J, int32_t h0,
                               void* state, size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    StreamDevice on_stream_device(stream);
    if (B < 0 || T <= 0 || P_r < 0 || F <= 0 || J <= 0 || h0 < 0) return fail(PAFUSE_E_ARG, "procrustes_partials: bad size");
    if (J > P2_MAX_J) return fail(PAFUSE_E_SHAPE, "procrustes_partials: J = %d above the supported %d", J, P2_MAX_J);
    if (int rc = check_state("procrustes_partials", state, state_bytes, pafuse_procrustes_partials_bytes(B, T, P_r, F, J))) return rc;
    const int64_t n = (int64_t)B * T * F * J;
    const P2StateViews v(state, n);
    hipStream_t s = (hipStream_t)stream;
    if (B == 0 || P_r == 0) return neutral_state("procrustes_partials", v, n, (size_t)P_r * T * 8, s);   // no kernel runs
    if (!pred || !gt || !x2d || !traj || !cam || !conn) return fail(PAFUSE_E_ARG, "procrustes_partials: null pointer");
    const size_t wneed = pafuse_procrustes_partials_workspace_bytes(B, T, P_r, F, J);
    if (!workspace || workspace_bytes < wneed || (uintptr_t)workspace % 8)
        return fail(PAFUSE_E_WORKSPACE, "procrustes_partials: the workspace needs %zu bytes, 8-byte aligned", wneed);
    const int64_t blocks = (int64_t)B * T * F;
    if (blocks > 0x7fffffff || (int64_t)P_r * T > 0x7fffffff || (int64_t)B * F > 0x7fffffff)
        return fail(PAFUSE_E_ARG, "procrustes_partials: grid out of range");
    ProcrustesPartialsParams m{};
    m.pred = pred, m.gt = gt, m.x2d = x2d, m.traj = traj, m.cam = cam, m.conn = conn;
    m.st = v, m.pose_sums = (double*)workspace;
    m.B = B, m.T = T, m.P = P_r, m.F = F, m.J = J, m.h0 = h0;
    int rc = launch<procrustes_partials_kernel>("procrustes_partials_kernel", (unsigned)blocks, 64 * P2_WAVES, 0, s, m);
    if (rc) return rc;
    ProcrustesPsumParams r{};
    r.pose_sums = m.pose_sums, r.psum = v.psum, r.B = B, r.T = T, r.P = P_r, r.F = F;
    return launch<procrustes_psum_kernel>("procrustes_psum_kernel", (unsigned)((int64_t)P_r * T), 256, 0, s, r);
}

int pafuse_procrustes_combine(const void* states, int32_t W, size_t stride_bytes, const void* sums, size_t sums_stride_bytes,
                              const float* gt, const int32_t* conn, int32_t B, int32_t T, int32_t F, int32_t J,
                              int32_t P_total, void* merged, float* jbest, float* pagg, float* jagg, int32_t* pick,
                              void* stream) {
    StreamDevice on_stream_device(stream);
    if (B < 0 || T <= 0 || F <= 0 || J <= 0 || W < 1) return fail(PAFUSE_E_ARG, "procrustes_combine: bad size");
    if (P_total < 1) return fail(PAFUSE_E_ARG, "procrustes_combine: P_total %d", P_total);
    if (J > P2_MAX_J) return fail(PAFUSE_E_SHAPE, "procrustes_combine: J = %d above the supported %d", J, P2_MAX_J);
    if (!merged && !jbest && !pagg && !jagg && !pick) return fail(PAFUSE_E_ARG, "procrustes_combine: nothing to write");
    if (pagg && !sums) return fail(PAFUSE_E_ARG, "procrustes_combine: pagg needs the sums of the mean pose");
    const int64_t n = (int64_t)B * T * F * J;
    if (n == 0) return PAFUSE_OK;
    if (!states || (pagg && (!gt || !conn))) return fail(PAFUSE_E_ARG, "procrustes_combine: null pointer");
    const int64_t blocks = ((int64_t)B * T * F + P2C_WAVES - 1) / P2C_WAVES;
    const size_t head = P2StateViews::head_bytes(n), sums_bytes = (size_t)n * 3 * sizeof(double);   // double sum[n][3] heads every row of sums
    if (int rc = check_combine("procrustes_combine", states, W, stride_bytes, head, merged, MergeOver::First, blocks)) return rc;
    if (pagg && (sums_stride_bytes < sums_bytes || sums_stride_bytes % 8 || (uintptr_t)sums % 8))
        return fail(PAFUSE_E_ARG, "procrustes_combine: sums are %zu bytes or more apart, 8-byte aligned", sums_bytes);
    if (merged && pagg) {
        const char *mg = (const char*)merged, *slo = (const char*)sums;
        const char* shi = slo + (size_t)(W - 1) * sums_stride_bytes + sums_bytes;
        if (mg < shi && mg + head > slo) return fail(PAFUSE_E_ARG, "procrustes_combine: the merged state lies over the sums");
    }
    ProcrustesCombineParams c{};
    c.states = (const char*)states, c.stride = (int64_t)stride_bytes, c.W = W, c.gt = gt, c.conn = conn;
    c.sums = pagg ? (const char*)sums : nullptr, c.sums_stride = (int64_t)sums_stride_bytes;
    if (merged) c.merged = P2StateViews(merged, n);
    c.jbest = jbest, c.pagg = pagg, c.jagg = jagg, c.pick = pick;
    c.B = B, c.T = T, c.F = F, c.J = J, c.P = P_total;
    return launch<procrustes_combine_kernel>("procrustes_combine_kernel", (unsigned)blocks, 64 * P2C_WAVES, 0, (hipStream_t)stream, c);
}

int pafuse_d3dp_replay_gemms(const pafuse_d3dp_config* cfg, int32_t B, int32_t P, void* workspace,
                             size_t workspace_bytes, void* stream, double* flops) {
    return pafuse_d3dp_replay_layers(cfg, B, P, workspace, workspace_bytes, stream, 15, flops);
}

int pafuse_d3dp_replay_layers(const pafuse_d3dp_config* cfg, int32_t B, int32_t P, void* workspace,
                              size_t workspace_bytes, void* stream, int32_t layer_mask, double* flops) {
    StreamDevice on_stream_device(stream);
    if (layer_mask < 1 || layer_mask > 15) return fail(PAFUSE_E_ARG, "replay_layers: layer_mask %d", layer_mask);
    int rc = d3dp_check(cfg, B, P);
    if (rc) return rc;
    if (!workspace || workspace_bytes < pafuse_d3dp_workspace_bytes(cfg, B, P))
        return fail(PAFUSE_E_WORKSPACE, "workspace too small");
    const int nflip = cfg->flip ? 2 : 1;
    const int64_t R = (int64_t)nflip * B * P;
    char* base = (char*)workspace + align_up((size_t)B * P * cfg->frames * cfg->num_kps * 3 * 4);
    int launches = 0;
    double fl = 0.0;
    PartBuffers pb[PAFUSE_MAX_PARTS];
    const pafuse_mixste2_weights* ws[PAFUSE_MAX_PARTS];
    int64_t Rs[PAFUSE_MAX_PARTS];
    for (int i = 0; i < cfg->num_parts; ++i) {
        base = carve_part(base, R * cfg->frames * cfg->part[i].joints, cfg->part[i].channels, B, pb[i], image_elem_bytes(cfg->part[i].operand_bf16));
        ws[i] = &cfg->part[i], Rs[i] = R;
    }
    if (parts_groupable(cfg)) {  // the schedule pafuse_d3dp_sample runs: block k of every part in shared grids
        if ((rc = run_mixste_layers_n(ws, pb, Rs, cfg->num_parts, (hipStream_t)stream, true, &fl, &launches, layer_mask)))
            return rc;
    } else {
        for (int i = 0; i < cfg->num_parts; ++i)
            if ((rc = run_mixste_layers(&cfg->part[i], pb[i], R, (hipStream_t)stream, true, &fl, &launches, layer_mask)))
                return rc;
    }
    if (flops) *flops += fl;
    return launches;
}

// ------------------------------------------------------------------------------------------------- training
int pafuse_attention_backward(const float* qkv, const float* d_o, float* dqkv, int64_t nseq, int32_t L, int32_t C, int32_t heads,
                              int64_t group, int64_t group_stride, int64_t seq_stride, int64_t tok_stride, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!qkv || !d_o || !dqkv || nseq < 0 || heads <= 0 || C % heads || group <= 0 || L <= 0)
        return fail(PAFUSE_E_ARG, "attention_backward: bad argument");
    if ((C / heads) % 4) return fail(PAFUSE_E_SHAPE, "attention_backward: head width %d must be a multiple of 4", C / heads);
    if (nseq == 0) return PAFUSE_OK;
    AttnBackwardParams ab{};
    ab.qkv = qkv, ab.d_o = d_o, ab.dqkv = dqkv, ab.nseq = nseq, ab.group = group, ab.group_stride = group_stride;
    ab.seq_stride = seq_stride, ab.tok_stride = tok_stride, ab.L = L, ab.C = C, ab.heads = heads, ab.d = C / heads;
    ab.scale = 1.0f / sqrtf((float)(C / heads));
    return attention_backward(ab, (hipStream_t)stream);
}

size_t pafuse_linear_weight_grad_bytes(void) { return TRAIN_PARTIAL_FLOATS * sizeof(float); }

int pafuse_linear_weight_grad(const float* dY, const float* X, float* dW, float* db, int64_t M, int32_t N, int32_t K,
                              int32_t operand_bf16, void* workspace, size_t workspace_bytes, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!dY || !X || !dW || !workspace || M < 0 || N <= 0 || K <= 0) return fail(PAFUSE_E_ARG, "linear_weight_grad: bad argument");
    if (operand_bf16 != MODE_F32 && operand_bf16 != MODE_BF16X3) return fail(PAFUSE_E_ARG, "linear_weight_grad: matrix-product mode %d (0 or 2)", operand_bf16);
    if (N % 4 || K % 4) return fail(PAFUSE_E_SHAPE, "linear_weight_grad: N=%d K=%d must be multiples of 4", N, K);
    if (workspace_bytes < pafuse_linear_weight_grad_bytes()) return fail(PAFUSE_E_WORKSPACE, "workspace too small");
    if (M == 0) return PAFUSE_OK;
    TrainBuffers tb{};
    tb.split = operand_bf16 == MODE_BF16X3;
    tb.partial = tb.partial_side = (float*)workspace;
    tb.partial_floats = TRAIN_PARTIAL_FLOATS;
    return weight_grad(dY, X, dW, M, N, K, tb, (hipStream_t)stream, false, db);
}

// workspace of the unit entries below, carved in this order (tb null: only the size): the column-sum partials of ln_backward /
// gelu_bwd (width max(N, K)), the transposed weight and the split image of a dX GEMM, its zero bias
static size_t carve_unit(char* base, int64_t M, int N, int K, TrainBuffers* tb) {
    const size_t W = (size_t)std::max(N, K);
    const size_t parts = std::max((size_t)blocks_for(M, LNB_ROWS_PER_BLOCK) * 3 * W, (size_t)std::min<int64_t>(1024, (M + 31) / 32) * W);
    const size_t part_b = align_up(parts * 4), wt_b = align_up((size_t)N * K * 4), img_b = align_up((size_t)N * K * 6);
    if (tb) {
        *tb = TrainBuffers{};
        tb->partial = tb->partial_side = (float*)base, tb->partial_floats = parts;
        tb->wt = (float*)(base + part_b), tb->wimg = (uint8_t*)(base + part_b + wt_b), tb->zeros = (float*)(base + part_b + wt_b + img_b);
    }
    return part_b + wt_b + img_b + align_up(W * 4);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }   // (null: nothing is loaded)

size_t pafuse_train_unit_bytes(int64_t M, int32_t N, int32_t K) {
    return (M < 0 || N < 0 || K < 0) ? 0 : carve_unit(nullptr, M, N, K, nullptr);
}

int pafuse_layernorm_backward(const pafuse_lnb_args* a, void* workspace, size_t workspace_bytes, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!a || !a->dy || !a->x || !a->w || !a->dx || !a->dw || !a->db || !workspace || a->M < 0)
        return fail(PAFUSE_E_ARG, "layernorm_backward: null pointer or negative M");
    if (a->C < 1 || a->C > LN_BACKWARD_MAX_C) return fail(PAFUSE_E_SHAPE, "layernorm_backward: C=%d outside 1 .. %d", a->C, LN_BACKWARD_MAX_C);
    if (a->dbranch && !a->out_scaled) return fail(PAFUSE_E_ARG, "layernorm_backward: dbranch without out_scaled");
    if (a->drop && (a->J <= 0 || (a->temporal && a->FJ <= 0)))
        return fail(PAFUSE_E_ARG, "layernorm_backward: drop with J=%d, FJ=%d", a->J, a->FJ);
    if (!aligned16(workspace) || (ln_backward_quad(a->C) && !(aligned16(a->dy) && aligned16(a->x) && aligned16(a->w) &&
                                                              aligned16(a->add) && aligned16(a->dx) && aligned16(a->out_scaled))))
        return fail(PAFUSE_E_ARG, "layernorm_backward: a tensor read with 16-byte accesses is not 16-byte aligned (C=%d)", a->C);
    if (workspace_bytes < carve_unit(nullptr, a->M, a->C, 0, nullptr)) return fail(PAFUSE_E_WORKSPACE, "layernorm_backward: workspace too small");
    if (a->M == 0) return PAFUSE_OK;
    TrainBuffers tb;
    carve_unit((char*)workspace, a->M, a->C, 0, &tb);
    return ln_backward(a->dy, a->x, a->w, a->eps, a->add, a->dx, a->drop, SeqMap{a->temporal, a->J, a->FJ}, a->out_scaled,
                       a->dw, a->db, a->dbranch, a->M, a->C, tb, (hipStream_t)stream);
}

int pafuse_linear_input_grad(const float* dY, const float* W, const float* dact_u, float* dX, int64_t M, int32_t N, int32_t K,
                             int32_t operand_bf16, int32_t image_source, void* workspace, size_t workspace_bytes, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!dY || !W || !dX || !workspace || M < 0) return fail(PAFUSE_E_ARG, "linear_input_grad: null pointer or negative M");
    if (operand_bf16 != MODE_F32 && operand_bf16 != MODE_BF16X3) return fail(PAFUSE_E_ARG, "linear_input_grad: matrix-product mode %d (0 or 2)", operand_bf16);
    if (image_source != 0 && image_source != 1) return fail(PAFUSE_E_ARG, "linear_input_grad: image source %d (0 or 1)", image_source);
    if (N <= 0 || K <= 0 || N % 32 || K % 32) return fail(PAFUSE_E_SHAPE, "linear_input_grad: N=%d, K=%d must be positive multiples of 32", N, K);
    const bool split = operand_bf16 == MODE_BF16X3 && plain_splits(M, K, N);
    if (dact_u && !split && K % 64) return fail(PAFUSE_E_SHAPE, "linear_input_grad: dact_u on fp32 products needs K %% 64 == 0, K=%d", K);
    if (!aligned16(dY) || !aligned16(W) || !aligned16(dact_u) || !aligned16(dX) || !aligned16(workspace))
        return fail(PAFUSE_E_ARG, "linear_input_grad: an operand is not 16-byte aligned");
    if (workspace_bytes < carve_unit(nullptr, M, N, K, nullptr)) return fail(PAFUSE_E_WORKSPACE, "linear_input_grad: workspace too small");
    if (M == 0) return PAFUSE_OK;
    TrainBuffers tb;
    carve_unit((char*)workspace, M, N, K, &tb);
    tb.split = operand_bf16 == MODE_BF16X3;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(tb.zeros, 0, (size_t)K * 4, s) != hipSuccess) return fail(PAFUSE_E_HIP, "memset failed");
    const uint8_t* image = nullptr;
    if (split && image_source == 1) {   // the image as the step makes it: one item of the batch kernel (prepare_images)
        SplitBatchParams p{};
        const int blocks = add_split_item(p, 0, W, tb.wimg, N, K, transposed_split_kind(K));
        const int rc = launch<split_weights_batch_kernel>("split_weights_batch_kernel", (unsigned)blocks, 256, 0, s, p);
        if (rc) return rc;
        image = tb.wimg;
    }
    return input_grad(dY, W, dX, M, N, K, tb, s, dact_u, image);
}

int pafuse_linear_train(const float* A, const float* W, const float* bias, float* u, float* h, int64_t M, int32_t N, int32_t K,
                        int32_t operand_bf16, void* workspace, size_t workspace_bytes, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!A || !W || !bias || !u || !workspace || M < 0) return fail(PAFUSE_E_ARG, "linear_train: null pointer or negative M");
    if (operand_bf16 != MODE_F32 && operand_bf16 != MODE_BF16X3) return fail(PAFUSE_E_ARG, "linear_train: matrix-product mode %d (0 or 2)", operand_bf16);
    if (N <= 0 || K <= 0 || N % 32 || K % 32) return fail(PAFUSE_E_SHAPE, "linear_train: N=%d, K=%d must be positive multiples of 32", N, K);
    const bool split = operand_bf16 == MODE_BF16X3 && plain_splits(M, N, K);
    if (h && !split && N % 64) return fail(PAFUSE_E_SHAPE, "linear_train: h on fp32 products needs N %% 64 == 0, N=%d", N);
    if (!aligned16(A) || !aligned16(W) || !aligned16(bias) || !aligned16(u) || !aligned16(h) || !aligned16(workspace))
        return fail(PAFUSE_E_ARG, "linear_train: an operand is not 16-byte aligned");
    if (workspace_bytes < carve_unit(nullptr, M, N, K, nullptr)) return fail(PAFUSE_E_WORKSPACE, "linear_train: workspace too small");
    if (M == 0) return PAFUSE_OK;
    TrainBuffers tb;
    carve_unit((char*)workspace, M, N, K, &tb);
    tb.split = operand_bf16 == MODE_BF16X3;
    return plain_linear(A, W, bias, u, M, N, K, (hipStream_t)stream, &tb, h);
}

int pafuse_gelu_backward(const float* u, const float* dh, float* du, float* db, int64_t M, int32_t N, void* workspace,
                         size_t workspace_bytes, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!u || !dh || !du || !db || !workspace || M < 0) return fail(PAFUSE_E_ARG, "gelu_backward: null pointer or negative M");
    if (N <= 0 || N % 4) return fail(PAFUSE_E_SHAPE, "gelu_backward: N=%d must be a positive multiple of 4", N);
    if (!aligned16(u) || !aligned16(dh) || !aligned16(du) || !aligned16(workspace))
        return fail(PAFUSE_E_ARG, "gelu_backward: an operand is not 16-byte aligned");
    if (workspace_bytes < carve_unit(nullptr, M, N, 0, nullptr)) return fail(PAFUSE_E_WORKSPACE, "gelu_backward: workspace too small");
    if (M == 0) return PAFUSE_OK;
    TrainBuffers tb;
    carve_unit((char*)workspace, M, N, 0, &tb);
    return gelu_bwd(u, dh, du, db, M, N, tb, (hipStream_t)stream);
}

// Unit entries of the first- and last-layer gradients.  Their workspaces hold exactly what the host helpers write: the partials
// (row_chunks / group_chunks parts), and for the patch embedding the [M,5] input and the [5,C] sums in front of them.
static size_t head_grad_partials(int64_t M, int C) {
    int64_t rows;
    return M > 0 ? (size_t)row_chunks(M, rows) * 3 * C : 0;
}

static size_t group_sum_partials(int mode, int B, int F, int J, int C) {
    int per;
    const int count = group_sum_count(mode, B, F, J);
    return count > 0 ? (size_t)group_chunks(count, per) * group_sum_groups(mode, B, F, J) * C : 0;
}

static size_t patch_grad_partials(int B, int F, int J, int C) {
    const int64_t M = (int64_t)B * F * J;
    int64_t rows;
    if (M <= 0) return 0;
    return std::max((size_t)row_chunks(M, rows) * 5 * C, std::max(group_sum_partials(0, B, F, J, C), group_sum_partials(2, B, F, J, C)));
}

// B, F, J >= 0 and C >= 1 with B F J rows that the kernels' int row counts hold
static bool rim_dims_ok(int B, int F, int J, int C) { return B >= 0 && F >= 0 && J >= 0 && C >= 1; }
static bool rim_rows_fit(int B, int F, int J) {   // (a zero size leaves the other two's product in a group's int row count)
    const int64_t lim = 0x7fffffff;
    return (int64_t)B * F * J <= lim && (int64_t)B * F <= lim && (int64_t)B * J <= lim && (int64_t)F * J <= lim;
}

size_t pafuse_train_head_grad_bytes(int64_t M, int32_t C) {
    return (M < 0 || C < 1 || M > (int64_t)0xffffffff / C) ? 0 : align_up(head_grad_partials(M, C) * 4);
}

int pafuse_train_head_grad(const float* dout, const float* hn, const float* head_w, float* d_head_w, float* d_head_b, float* dhn,
                           int64_t M, int32_t C, void* workspace, size_t workspace_bytes, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!dout || !hn || !head_w || !d_head_w || !d_head_b || !dhn || !workspace || M < 0)
        return fail(PAFUSE_E_ARG, "train_head_grad: null pointer or negative M");
    // (head_backward_kernel: one thread per element of dhn, M C / 256 workgroups in one grid dimension)
    if (C < 1 || M > (int64_t)0xffffffff / C) return fail(PAFUSE_E_SHAPE, "train_head_grad: M=%lld, C=%d out of range", (long long)M, C);
    if (workspace_bytes < pafuse_train_head_grad_bytes(M, C)) return fail(PAFUSE_E_WORKSPACE, "train_head_grad: workspace too small");
    if (M == 0) return PAFUSE_OK;
    TrainBuffers tb{};
    tb.partial = tb.partial_side = (float*)workspace, tb.partial_floats = head_grad_partials(M, C);
    return head_grad(dout, hn, head_w, d_head_w, d_head_b, dhn, M, C, tb, (hipStream_t)stream);
}

size_t pafuse_train_patch_grad_bytes(int32_t B, int32_t F, int32_t J, int32_t C) {
    if (!rim_dims_ok(B, F, J, C) || !rim_rows_fit(B, F, J)) return 0;
    return align_up((size_t)B * F * J * 5 * 4) + align_up((size_t)5 * C * 4) + align_up(patch_grad_partials(B, F, J, C) * 4);
}

int pafuse_train_patch_grad(const float* x2d, const float* x3d, const float* g, float* d_patch_w, float* d_patch_b,
                            float* d_pos_spatial, float* dtemb, int32_t B, int32_t F, int32_t J, int32_t C, void* workspace,
                            size_t workspace_bytes, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!x2d || !x3d || !g || !d_patch_w || !d_patch_b || !d_pos_spatial || !dtemb || !workspace || B < 0 || F < 0 || J < 0)
        return fail(PAFUSE_E_ARG, "train_patch_grad: null pointer or negative size");
    if (C < 1 || !rim_rows_fit(B, F, J)) return fail(PAFUSE_E_SHAPE, "train_patch_grad: B=%d F=%d J=%d C=%d out of range", B, F, J, C);
    if (workspace_bytes < pafuse_train_patch_grad_bytes(B, F, J, C)) return fail(PAFUSE_E_WORKSPACE, "train_patch_grad: workspace too small");
    const int64_t M = (int64_t)B * F * J;
    if (M == 0) return PAFUSE_OK;
    hipStream_t s = (hipStream_t)stream;
    TrainBuffers tb{};
    char* base = (char*)workspace;
    tb.in5 = (float*)base, base += align_up((size_t)M * 5 * 4);
    tb.small = (float*)base, base += align_up((size_t)5 * C * 4);
    tb.partial = tb.partial_side = (float*)base, tb.partial_floats = patch_grad_partials(B, F, J, C);
    const int rc = concat_inputs(x2d, x3d, tb.in5, M, s);
    if (rc) return rc;
    return patch_grad(tb.in5, g, d_patch_w, d_patch_b, d_pos_spatial, dtemb, B, F, J, C, tb, s);
}

size_t pafuse_train_group_sum_bytes(int32_t mode, int32_t B, int32_t F, int32_t J, int32_t C) {
    if (mode < 0 || mode > 2 || !rim_dims_ok(B, F, J, C) || !rim_rows_fit(B, F, J)) return 0;
    return align_up(group_sum_partials(mode, B, F, J, C) * 4);
}

int pafuse_train_group_sum(const float* x, float* out, int32_t mode, int32_t accumulate, int32_t B, int32_t F, int32_t J, int32_t C,
                           void* workspace, size_t workspace_bytes, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!x || !out || !workspace || B < 0 || F < 0 || J < 0) return fail(PAFUSE_E_ARG, "train_group_sum: null pointer or negative size");
    if (mode < 0 || mode > 2) return fail(PAFUSE_E_ARG, "train_group_sum: mode %d (0, 1 or 2)", mode);
    if (accumulate != 0 && accumulate != 1) return fail(PAFUSE_E_ARG, "train_group_sum: accumulate %d (0 or 1)", accumulate);
    if (C < 1 || !rim_rows_fit(B, F, J)) return fail(PAFUSE_E_SHAPE, "train_group_sum: B=%d F=%d J=%d C=%d out of range", B, F, J, C);
    if (workspace_bytes < pafuse_train_group_sum_bytes(mode, B, F, J, C)) return fail(PAFUSE_E_WORKSPACE, "train_group_sum: workspace too small");
    if ((int64_t)B * F * J == 0) return PAFUSE_OK;
    TrainBuffers tb{};
    tb.partial = tb.partial_side = (float*)workspace, tb.partial_floats = group_sum_partials(mode, B, F, J, C);
    return group_sum(x, out, mode, B, F, J, C, tb, (hipStream_t)stream, accumulate);
}

int pafuse_train_sinusoid(const int64_t* t, const float* freqs, float* out, int32_t B, int32_t C, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!t || !freqs || !out || B < 0) return fail(PAFUSE_E_ARG, "train_sinusoid: null pointer or negative B");
    if (C < 2 || C % 2 || (int64_t)B * C > 0x7fffffff) return fail(PAFUSE_E_SHAPE, "train_sinusoid: C=%d must be even and positive (B=%d)", C, B);
    if (B == 0) return PAFUSE_OK;
    return sinusoid(t, freqs, out, B, C, (hipStream_t)stream);
}

size_t pafuse_mixste2_train_bytes(const pafuse_mixste2_weights* w, int32_t B) {
    if (!w || B <= 0 || check_weights(w, true)) return 0;
    return train_bytes(w, B);
}

int pafuse_mixste2_train_forward(const pafuse_mixste2_weights* w, const float* x2d, const float* x3d, const int64_t* t,
                                 int32_t B, const float* drop_path, float* out, void* saved, size_t saved_bytes,
                                 void* stream) {
    StreamDevice on_stream_device(stream);
    int rc = check_weights(w, true);
    if (rc) return rc;
    if (!x2d || !x3d || !t || !out || !saved || B <= 0) return fail(PAFUSE_E_ARG, "mixste2_train_forward: bad argument");
    if ((w->mlp_hidden && w->mlp_hidden != 2 * w->channels) || w->qk_scale != 0.f)
        return fail(PAFUSE_E_SHAPE, "training implements the PAFUSE configuration only (mlp_ratio = 2, qk_scale = None)");
    // (the spatial sequences stay within the short attention backward kernels; the temporal ones may use the long one)
    if (w->joints > 80 || w->frames > ATTN_BWD_LONG_LP)
        return fail(PAFUSE_E_SHAPE, "training: sequence lengths J=%d F=%d must be <= 80 / <= %d (the single-model variant is inference only)",
                    w->joints, w->frames, ATTN_BWD_LONG_LP);
    if (!train_partials_fit(w, B)) return fail(PAFUSE_E_SHAPE, "training: B=%d exceeds the %d samples per call at width %d", B, train_max_batch(w), w->channels);
    if (saved_bytes < train_bytes(w, B)) return fail(PAFUSE_E_WORKSPACE, "mixste2_train_forward: buffer too small");
    TrainBuffers tb;
    carve_train((char*)saved, w, B, tb);
    return train_forward(w, x2d, x3d, t, B, drop_path, out, tb, (hipStream_t)stream);
}

int pafuse_mixste2_train_backward(const pafuse_mixste2_weights* w, const pafuse_mixste2_weights* grads, const float* dout,
                                  int32_t B, const float* drop_path, void* saved, size_t saved_bytes, void* stream,
                                  void* side_stream) {
    StreamDevice on_stream_device(stream);
    int rc = check_weights(w, true);
    if (rc) return rc;
    if (!grads || !dout || !saved || B <= 0) return fail(PAFUSE_E_ARG, "mixste2_train_backward: bad argument");
    if (!train_partials_fit(w, B)) return fail(PAFUSE_E_SHAPE, "training: B=%d exceeds the %d samples per call at width %d", B, train_max_batch(w), w->channels);
    if (saved_bytes < train_bytes(w, B)) return fail(PAFUSE_E_WORKSPACE, "mixste2_train_backward: buffer too small");
    TrainBuffers tb;
    carve_train((char*)saved, w, B, tb);
    return train_backward(w, grads, dout, B, drop_path, tb, (hipStream_t)stream, (hipStream_t)side_stream);
}

int pafuse_d3dp_qsample(const float* x0, const float* noise, const int64_t* t, const double* sqrt_alphas_cumprod,
                        const double* sqrt_one_minus_alphas_cumprod, double scale, float* out, int32_t B,
                        int64_t per_sample, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!x0 || !noise || !t || !sqrt_alphas_cumprod || !sqrt_one_minus_alphas_cumprod || !out || B <= 0 || per_sample <= 0)
        return fail(PAFUSE_E_ARG, "d3dp_qsample: bad argument");
    QsampleParams q{};
    q.x0 = x0, q.noise = noise, q.t = t, q.sqrt_acp = sqrt_alphas_cumprod, q.sqrt_1m_acp = sqrt_one_minus_alphas_cumprod;
    q.scale = scale, q.out = out, q.per_sample = per_sample, q.n = (int64_t)B * per_sample;
    return launch<qsample_kernel>("qsample_kernel", blocks_for(q.n), 256, 0, (hipStream_t)stream, q);
}

int pafuse_d3dp_qsample_seeded(const float* x0, const uint32_t* key4_dev, const double* sqrt_alphas_cumprod,
                               const double* sqrt_one_minus_alphas_cumprod, double scale, int32_t num_timesteps, float* out,
                               int64_t* t_out, float* noise_out, int32_t B, int32_t F, int32_t J, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!x0 || !key4_dev || !sqrt_alphas_cumprod || !sqrt_one_minus_alphas_cumprod || !out || !t_out)
        return fail(PAFUSE_E_ARG, "d3dp_qsample_seeded: null pointer");
    if (num_timesteps <= 0 || B <= 0 || F <= 0 || J <= 0)
        return fail(PAFUSE_E_ARG, "d3dp_qsample_seeded: bad size (num_timesteps=%d B=%d F=%d J=%d)", num_timesteps, B, F, J);
    const int64_t threads = (int64_t)B * F * J;
    if ((int64_t)F * J > 0xffffffffLL || (threads + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "d3dp_qsample_seeded: size out of range");
    QsampleParams q{};
    q.x0 = x0, q.key4 = key4_dev, q.num_timesteps = (uint32_t)num_timesteps, q.t_out = t_out, q.noise_out = noise_out;
    q.sqrt_acp = sqrt_alphas_cumprod, q.sqrt_1m_acp = sqrt_one_minus_alphas_cumprod;
    q.scale = scale, q.out = out, q.per_sample = (int64_t)F * J * 3, q.n = threads * 3;
    return launch<qsample_seeded_kernel>("qsample_seeded_kernel", blocks_for(threads), 256, 0, (hipStream_t)stream, q);
}

int pafuse_train_droppath_fill(const uint32_t* key4_dev, int32_t denoiser, int32_t depth, int32_t F, int32_t J, int32_t B,
                               const double* keep, const float* factor, float* out, int64_t out_floats, void* stream) {
    StreamDevice on_stream_device(stream);
    if (!key4_dev || !keep || !factor || !out) return fail(PAFUSE_E_ARG, "train_droppath_fill: null pointer");
    if (denoiser < 0 || denoiser >= (1 << 16) || depth <= 0 || depth > (1 << 14) || B <= 0 || F <= 0 || J <= 0)
        return fail(PAFUSE_E_ARG, "train_droppath_fill: bad argument (denoiser=%d depth=%d B=%d F=%d J=%d)", denoiser, depth, B, F, J);
    const int64_t n = 4 * (int64_t)depth * B * (F > J ? F : J);
    if ((int64_t)F * J > 0xffffffffLL || (n + 255) / 256 > 0x7fffffff) return fail(PAFUSE_E_ARG, "train_droppath_fill: size out of range");
    if (out_floats < n) return fail(PAFUSE_E_ARG, "train_droppath_fill: out holds %lld floats, the table has %lld", (long long)out_floats, (long long)n);
    return launch<droppath_fill_kernel>("droppath_fill_kernel", blocks_for(n), 256, 0, (hipStream_t)stream, key4_dev, (uint32_t)denoiser, depth, F, J, B,
                                        keep, factor, out);
}

}  // extern "C"
