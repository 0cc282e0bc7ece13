// train_host.inc - host side of the training entry points (included by pafuse_hip.hip inside its anonymous namespace,
// after the inference helpers it reuses: gemm_bias, attention, check_weights, align_up, fail, launch).
//
// Train-mode MixSTE2 (common/mixste.py:215-225,260-298) is the inference network at P = 1 plus DropPath on both
// residual branches of every block; the forward runs the inference kernels (whole-row epilogues in their
// EPI_ROWLN_TRAIN form) and keeps what the backward needs, the backward walks the blocks in reverse.
// Linear layers: dX through the inference GEMM on a transposed weight copy, dW through tn_gemm_kernel.

struct TrainBlockBuffers {
    float *x_in, *xn1, *qkv, *o, *x1, *xn2, *u, *h, *x2;  // [M,C] except qkv [M,3C], u and h = gelu(u) [M,2C]
};

struct TrainBuffers {
    TrainBlockBuffers blk[2 * PAFUSE_MAX_DEPTH];
    float *y_last, *hn;                // [M,C]: output of the last block, head LayerNorm output
    float* in5;                        // [M,5]
    float *sincos, *uh, *hid, *temb;   // time MLP: [B,C], [B,2C], [B,2C], [B,C]
    float *g, *g2, *dscaled, *e;       // [M,C] scratch
    float *big1, *big2;                // [M,3C] scratch
    float *wt;                         // [3C*C] transposed weight
    uint8_t *wimg;                     // [18 C*C bytes] split-precision image of a weight outside the blocks (made in front of its GEMM)
    uint8_t *wimg_blocks;              // [2 depth][48 C*C bytes] the images of the blocks' four linear weights, one launch per pass
    const uint8_t* img[2 * PAFUSE_MAX_DEPTH][4];   // qkv, proj, fc1, fc2 of block k in wimg_blocks (null: no image - fp32 products)
    bool split;                        // MODE_BF16X3: the plain GEMMs (qkv, fc1, every dX) run bf16x3 products
    float *zeros;                      // [3C] zero bias of the dX GEMMs
    float *small;                      // [max(B,8) * 2C] tiny results (d temb, d hid, [5][C] sums)
    float *partial, *partial_side;     // two-stage reduction partials (main stream / weight-gradient side stream)
    size_t partial_floats;
};

constexpr int TN_TARGET_WORKGROUPS = 512;  // ~2 per CU: more splits only add partial-sum traffic
// room for one large-tile workgroup per CU (256 x 256 outputs each) plus the column-sum partials: the partial tiles of a
// weight gradient are written once and read once - 67 MB per launch at 256 workgroups, beside the 170 - 340 MB its operands take
constexpr size_t TRAIN_PARTIAL_FLOATS = (size_t)(256 + 32) * 256 * 256;
// The small reductions of the first and last layers share it: the largest, group_sum, writes 32 chunks x max(B, F, J) groups x C
// floats - 6.3 M at F = 256, C = 768, whatever J <= 80.  Its per-sample mode bounds B: 32 B C floats, B <= 1536 at C = 384.
inline int train_max_batch(const pafuse_mixste2_weights* w) { return (int)(TRAIN_PARTIAL_FLOATS / ((size_t)32 * w->channels)); }
inline bool train_partials_fit(const pafuse_mixste2_weights* w, int B) {
    return (size_t)32 * std::max(B, std::max(w->frames, w->joints)) * w->channels <= TRAIN_PARTIAL_FLOATS;
}

size_t train_bytes(const pafuse_mixste2_weights* w, int B) {
    const size_t M = (size_t)B * w->frames * w->joints, C = w->channels;
    const size_t mc = align_up(M * C * 4);
    size_t total = (size_t)2 * w->depth * (6 * mc + align_up(M * 3 * C * 4) + 2 * align_up(M * 2 * C * 4));
    total += 2 * mc + align_up(M * 5 * 4);
    total += 2 * align_up((size_t)B * C * 4) + 2 * align_up((size_t)B * 2 * C * 4);
    total += 4 * mc + 2 * align_up(M * 3 * C * 4);
    total += align_up(3 * C * C * 4) + align_up(3 * C * 4) + align_up((size_t)std::max(B, 8) * 2 * C * 4);
    total += align_up(18 * C * C);   // wimg
    total += align_up((size_t)2 * w->depth * 48 * C * C);   // wimg_blocks (8 C^2 weights per block, 6 bytes each)
    total += 2 * align_up(TRAIN_PARTIAL_FLOATS * 4);
    return total;
}

void carve_train(char* base, const pafuse_mixste2_weights* w, int B, TrainBuffers& tb) {
    const size_t M = (size_t)B * w->frames * w->joints, C = w->channels;
    auto take = [&](size_t floats) {
        float* p = (float*)base;
        base += align_up(floats * 4);
        return p;
    };
    for (int k = 0; k < 2 * w->depth; ++k) {
        TrainBlockBuffers& b = tb.blk[k];
        b.x_in = take(M * C), b.xn1 = take(M * C), b.qkv = take(M * 3 * C), b.o = take(M * C);
        b.x1 = take(M * C), b.xn2 = take(M * C), b.u = take(M * 2 * C), b.h = take(M * 2 * C), b.x2 = take(M * C);
    }
    tb.y_last = take(M * C), tb.hn = take(M * C), tb.in5 = take(M * 5);
    tb.sincos = take((size_t)B * C), tb.temb = take((size_t)B * C);
    tb.uh = take((size_t)B * 2 * C), tb.hid = take((size_t)B * 2 * C);
    tb.g = take(M * C), tb.g2 = take(M * C), tb.dscaled = take(M * C), tb.e = take(M * C);
    tb.big1 = take(M * 3 * C), tb.big2 = take(M * 3 * C);
    tb.wt = take(3 * C * C), tb.zeros = take(3 * C), tb.small = take((size_t)std::max(B, 8) * 2 * C);
    tb.wimg = (uint8_t*)take((18 * C * C + 3) / 4);
    tb.wimg_blocks = (uint8_t*)take((size_t)2 * w->depth * 12 * C * C);
    for (int k = 0; k < 2 * PAFUSE_MAX_DEPTH; ++k) tb.img[k][0] = tb.img[k][1] = tb.img[k][2] = tb.img[k][3] = nullptr;
    tb.split = w->operand_bf16 == MODE_BF16X3;
    tb.partial = take(TRAIN_PARTIAL_FLOATS), tb.partial_side = take(TRAIN_PARTIAL_FLOATS);
    tb.partial_floats = TRAIN_PARTIAL_FLOATS;
}

// which GEMMs of the training step run split-precision (their weight needs an image)
inline bool plain_splits(int64_t M, int N, int K) { return M >= 128 && K % 32 == 0 && N % 32 == 0; }
// image layout of a plain split GEMM: 2 = the M16 image of the 16x16x32 kernels, for EVERY plain GEMM of the step since round 6 (rounds 3 - 5:
// the forward qkv layers and the face only) - they run the persistent strip kernel of inference (sgemm.hpp; its epilogue has training's
// two options: fc1 forward's out_act, fc2-dX's dact_u).  No kernel of the forward / dX GEMMs issues
// v_mfma_f32_32x32x16_bf16 any more except the whole-row forward tiles.  (-DPAFUSE_TRAIN_PLAIN_LAYOUT0: the old rule, for the A/B.)
#ifdef PAFUSE_TRAIN_PLAIN_LAYOUT0
inline int plain_layout(int N, bool qkv_forward) { return (qkv_forward || N % 224 == 0) ? WLAYOUT_M16 : WLAYOUT_PLAIN; }
#else
inline int plain_layout(int, bool) { return WLAYOUT_M16; }
#endif
inline bool rowln_splits(int64_t M, int N, int K) { return M >= 4096 && (N == 384 || N == 256 || N == 224) && K % 32 == 0; }

// whole-row GEMM of the training forward (proj / fc2 + DropPath row factor + LayerNorm chain): with split products the
// weight's whole-row image (layout 1) is made right here, as plain_linear does for the plain GEMMs
int rowln_train(GemmParams q, TrainBuffers& tb, hipStream_t s, const uint8_t* image = nullptr) {
    if (tb.split && rowln_splits(q.M, q.N, q.K)) {
        if (!image) {
            const int64_t n = (int64_t)q.N * (q.K / 8);
            int rc = launch<split_weights_kernel<16, 0>>("split_weights_kernel", blocks_for(n), 256, 0, s, q.W, tb.wimg, q.N, q.K);
            if (rc) return rc;
            image = tb.wimg;
        }
        q.mode = MODE_BF16X3, q.Wsplit = image;
    }
    return gemm_rowln_train(q, s);
}

// out = A W^T + bias.  With `tb` given and tb->split set (precision 'bf16x3' in training) the product runs split-precision on
// `image` (prepare_images) or, without one, on an image made right here (6 bytes per element into tb->wimg, stream-ordered
// with the GEMM that reads it) - fp32-equivalent products at 1.5x the fp32-matrix rate.
int plain_linear(const float* A, const float* W, const float* bias, float* out, int64_t M, int N, int K, hipStream_t s,
                 TrainBuffers* tb = nullptr, float* out_act = nullptr, const uint8_t* image = nullptr, bool qkv_forward = false) {
    GemmParams g{};
    g.A = A, g.W = W, g.bias = bias, g.out = out, g.M = M, g.N = N, g.K = K, g.act = 0, g.out_act = out_act;
    if (tb && tb->split && plain_splits(M, N, K)) {
        const int wl = plain_layout(N, qkv_forward);
        if (!image) {
            const int64_t n = (int64_t)N * (K / 8);
            const int rc = wl == WLAYOUT_M16 ? launch<split_weights_kernel<32, 1>>("split_weights_kernel", blocks_for(n), 256, 0, s, W, tb->wimg, N, K)
                                             : launch<split_weights_kernel<32, 0>>("split_weights_kernel", blocks_for(n), 256, 0, s, W, tb->wimg, N, K);
            if (rc) return rc;
            image = tb->wimg;
        }
        g.mode = MODE_BF16X3, g.Wsplit = image, g.wlayout = wl;
    }
    return gemm_bias(g, s);
}

int reduce_into(const float* partial, float* out, int n, int nparts, int64_t stride, hipStream_t s, int accumulate = 1,
                float* out2 = nullptr, int split = -1, float* out3 = nullptr, int split2 = 0) {
    if (split < 0) split = n;
    if (n >= 16384 || nparts < 32)
        return launch<reduce_partials_kernel<1>>("reduce_partials_kernel", blocks_for(n), 256, 0, s, partial, out, out2, split, n, nparts, stride,
                                                 accumulate, out3, split2);
    return launch<reduce_partials_kernel<16>>("reduce_partials_kernel", blocks_for(n, 16), 256, 0, s, partial, out, out2, split, n, nparts, stride,
                                              accumulate, out3, split2);
}

int bias_grad(const float* dY, float* db, int64_t M, int N, TrainBuffers& tb, hipStream_t s, bool side = false);

// the row split of the small reductions (bias_grad, outer_sum): chunks of `rows` rows, at most 256, none empty
inline int row_chunks(int64_t M, int64_t& rows) {
    const int chunks = (int)std::min<int64_t>(256, (M + 63) / 64);
    rows = (M + chunks - 1) / chunks;
    return (int)((M + rows - 1) / rows);
}
// the split of group_sum: chunks of `per` of a group's `count` rows, at most 32, none empty
inline int group_chunks(int count, int& per) {
    const int chunks = std::min(32, (count + 15) / 16);
    per = (count + chunks - 1) / chunks;
    return (count + per - 1) / per;
}
inline int group_sum_groups(int mode, int B, int F, int J) { return mode == 0 ? J : (mode == 1 ? F : B); }
inline int group_sum_count(int mode, int B, int F, int J) { return mode == 0 ? B * F : (mode == 1 ? B * J : F * J); }

constexpr int TN_BIG_TARGET_WORKGROUPS = 256;  // one large-tile workgroup per CU

template <int NB, int KB, int WN, int WK>
int launch_tn_big(const TnSplitParams& p, int tiles, int splits, hipStream_t s) {
    constexpr int lds = 2 * 3072 * (NB + KB);   // 72 - 96 KB
    return launch<tn_split_big_kernel<NB, KB, WN, WK>>("tn_split_big_kernel", dim3((unsigned)tiles, (unsigned)splits), 64 * WN * WK, lds, s, p);
}

// dW[N,K] += dY[M,N]^T X[M,K]; with db given also db[N] += column sums of dY (the bias gradient of the same Linear: with
// split products the weight-gradient kernel takes it from the values it stages anyway)
int weight_grad(const float* dY, const float* X, float* dW, int64_t M, int N, int K, TrainBuffers& tb, hipStream_t s,
                bool side = false, float* db = nullptr) {
    float* partial = side ? tb.partial_side : tb.partial;
    int rc;
    // large tiles where a PAFUSE width divides: 256 (hands), 192 (body), 224 (face)
    // (body: 384 x 128 tiles on eight waves - the 192 x 192 tile's six waves leave two of the four SIMDs with one wave)
    const int big = !tb.split || M < 4096 ? 0 : (N % 256 == 0 && K % 256 == 0 ? 256 : (N % 384 == 0 && K % 128 == 0 ? 384 :
                    (N % 192 == 0 && K % 192 == 0 ? 192 : (N % 224 == 0 && K % 224 == 0 ? 224 : 0))));
    if (big) {
        const int tiles = big == 384 ? (N / 384) * (K / 128) : (N / big) * (K / big);
        int splits = std::max(1, TN_BIG_TARGET_WORKGROUPS / tiles);
        splits = (int)std::min<size_t>((size_t)splits, tb.partial_floats / ((size_t)N * K + N));   // what the partial buffer holds
        if (splits < 1) return fail(PAFUSE_E_WORKSPACE, "weight_grad: partial buffer");
        const int64_t rows = ((M + splits - 1) / splits + 15) / 16 * 16;
        splits = (int)((M + rows - 1) / rows);
        if ((size_t)splits * N * K + (size_t)splits * N > tb.partial_floats) return fail(PAFUSE_E_WORKSPACE, "weight_grad: partial buffer");
        TnSplitParams p{};
        p.Y = dY, p.X = X, p.partial = partial, p.M = M, p.rows_per_split = rows, p.N = N, p.K = K;
        p.colsum = db ? partial + (size_t)splits * N * K : nullptr;
        rc = big == 256 ? launch_tn_big<8, 8, 4, 2>(p, tiles, splits, s)
           : big == 384 ? launch_tn_big<12, 4, 4, 2>(p, tiles, splits, s)
           : big == 192 ? launch_tn_big<6, 6, 3, 2>(p, tiles, splits, s) : launch_tn_big<7, 7, 7, 1>(p, tiles, splits, s);
        if (rc) return rc;
        if ((rc = reduce_into(partial, dW, N * K, splits, (int64_t)N * K, s))) return rc;
        return db ? reduce_into(p.colsum, db, N, splits, N, s) : PAFUSE_OK;
    }
    const int tiles = ((N + TN_BN - 1) / TN_BN) * ((K + TN_BK - 1) / TN_BK);
    int splits = (TN_TARGET_WORKGROUPS + tiles - 1) / tiles;
    int64_t rows = ((M + splits - 1) / splits + 31) / 32 * 32;
    if (rows < 32) rows = 32;
    splits = (int)((M + rows - 1) / rows);
    if ((size_t)splits * N * K + (size_t)splits * N > tb.partial_floats) return fail(PAFUSE_E_WORKSPACE, "weight_grad: partial buffer");
    if (tb.split && N % 2 == 0 && K % 2 == 0) {
        TnSplitParams p{};
        p.Y = dY, p.X = X, p.partial = partial, p.M = M, p.rows_per_split = rows, p.N = N, p.K = K;
        p.colsum = db ? partial + (size_t)splits * N * K : nullptr;
        if ((rc = launch<tn_split_gemm_kernel>("tn_split_gemm_kernel", dim3((unsigned)tiles, (unsigned)splits), 256, 0, s, p))) return rc;
        if ((rc = reduce_into(partial, dW, N * K, splits, (int64_t)N * K, s))) return rc;
        return db ? reduce_into(p.colsum, db, N, splits, N, s) : PAFUSE_OK;
    }
    TnParams p{};
    p.Y = dY, p.X = X, p.partial = partial, p.M = M, p.rows_per_split = rows, p.N = N, p.K = K;
    if ((rc = launch<tn_gemm_kernel>("tn_gemm_kernel", dim3((unsigned)tiles, (unsigned)splits), 256, 0, s, p))) return rc;   // fp32 products
    if ((rc = reduce_into(partial, dW, N * K, splits, (int64_t)N * K, s))) return rc;
    return db ? bias_grad(dY, db, M, N, tb, s, side) : PAFUSE_OK;
}

// db[N] += column sums of dY[M,N]
int bias_grad(const float* dY, float* db, int64_t M, int N, TrainBuffers& tb, hipStream_t s, bool side) {
    float* partial = side ? tb.partial_side : tb.partial;
    int64_t rows;
    const int chunks = row_chunks(M, rows);
    if ((size_t)chunks * N > tb.partial_floats) return fail(PAFUSE_E_WORKSPACE, "bias_grad: partial buffer");
    int rc = launch<colsum_kernel>("colsum_kernel", dim3(blocks_for(N), (unsigned)chunks), 256, 0, s, dY, partial, M, N, rows);
    if (rc) return rc;
    return reduce_into(partial, db, N, chunks, N, s);
}

// dX[M,K] = dY[M,N] W[N,K] through the inference GEMM on W^T; with split products the image of W^T is made from W as it lies
// (no transposed copy).  dact_u (may be null): dX is multiplied by gelu'(dact_u) in the epilogue (fc2: dX is d gelu(u)).
int input_grad(const float* dY, const float* W, float* dX, int64_t M, int N, int K, TrainBuffers& tb, hipStream_t s,
               const float* dact_u = nullptr, const uint8_t* image = nullptr) {
    GemmParams g{};
    g.A = dY, g.W = tb.wt, g.bias = tb.zeros, g.out = dX, g.M = M, g.N = K, g.K = N, g.act = 0, g.dact_u = dact_u;
    int rc;
    if (tb.split && plain_splits(M, K, N)) {
        const int wl = plain_layout(K, false);
        if (!image) {
            const int64_t n = (int64_t)K * (N / 8);
            rc = wl == WLAYOUT_M16 ? launch<split_weights_transposed_kernel<32, 1>>("split_weights_transposed_kernel", blocks_for(n), 256, 0, s, W, tb.wimg, K, N)
                                   : launch<split_weights_transposed_kernel<32, 0>>("split_weights_transposed_kernel", blocks_for(n), 256, 0, s, W, tb.wimg, K, N);
            if (rc) return rc;
            image = tb.wimg;
        }
        g.mode = MODE_BF16X3, g.Wsplit = image, g.wlayout = wl;
    } else {
        if ((rc = launch<transpose_kernel>("transpose_kernel", dim3(blocks_for(K, 32), blocks_for(N, 32)), 256, 0, s, W, tb.wt, N, K))) return rc;
    }
    return gemm_bias(g, s);
}

constexpr int LN_BACKWARD_MAX_C = 64 * LN_MAX_PER_LANE;
inline bool ln_backward_quad(int C) { return C % 4 == 0 && C <= 128 * LNB_NV; }

// dbranch (may be null): bias gradient of the Linear whose DropPath-scaled output joins the residual below this norm
// = column sums of out_scaled, accumulated alongside dw/db instead of a separate pass over [M,C]
int ln_backward(const float* dy, const float* x, const float* w, float eps, const float* add, float* dx,
                const float* drop, SeqMap map, float* out_scaled, float* dw, float* db, float* dbranch, int64_t M, int C,
                TrainBuffers& tb, hipStream_t s) {
    LnBackwardParams p{};
    p.dy = dy, p.x = x, p.w = w, p.eps = eps, p.add = add, p.dx = dx, p.drop = drop, p.map = map;
    p.out_scaled = out_scaled, p.partial = tb.partial, p.M = M, p.C = C;
    // (ln_backward_kernel keeps a row in LN_MAX_PER_LANE registers per lane: wider rows would lose channels and read past its LDS)
    if (C < 1 || C > LN_BACKWARD_MAX_C) return fail(PAFUSE_E_SHAPE, "ln_backward: C=%d outside 1 .. %d", C, LN_BACKWARD_MAX_C);
    const unsigned nb = blocks_for(M, LNB_ROWS_PER_BLOCK);
    if ((size_t)nb * 3 * C > tb.partial_floats) return fail(PAFUSE_E_WORKSPACE, "ln_backward: partial buffer");
    const int rc = ln_backward_quad(C) ? launch<ln_backward_quad_kernel>("ln_backward_kernel", nb, 256, 0, s, p)   // the PAFUSE widths: half-wave per row, 16-byte accesses
                                       : launch<ln_backward_kernel>("ln_backward_kernel", nb, 256, 0, s, p);
    if (rc) return rc;
    if (dbranch && out_scaled)   // dw, db and the branch's bias gradient in one pass over the partials
        return reduce_into(tb.partial, dw, 3 * C, (int)nb, 3 * (int64_t)C, s, 1, db, C, dbranch, 2 * C);
    return reduce_into(tb.partial, dw, 2 * C, (int)nb, 3 * (int64_t)C, s, 1, db, C);
}

int gelu_fwd(const float* u, float* h, int64_t n, hipStream_t s) {
    return launch<gelu_forward_kernel>("gelu_forward_kernel", blocks_for(n / 4), 256, 0, s, u, h, n / 4);
}

// du[M,N] = dh * gelu'(u) (in place allowed) and db[N] += column sums of du
int gelu_bwd(const float* u, const float* dh, float* du, float* db, int64_t M, int N, TrainBuffers& tb, hipStream_t s) {
    int chunks = (int)std::min<int64_t>(1024, (M + 31) / 32);
    const int64_t rows = (M + chunks - 1) / chunks;
    chunks = (int)((M + rows - 1) / rows);
    int rc = launch<gelu_backward_kernel>("gelu_backward_kernel", (unsigned)chunks, 256, 0, s, u, dh, du, tb.partial, M, N, rows);
    if (rc) return rc;
    return reduce_into(tb.partial, db, N, chunks, N, s);
}

// out[G][C] (+)= sums of x[B*F*J][C] over the rows of each group: mode 0 per joint, 1 per frame, 2 per sample (group_sum_kernel)
int group_sum(const float* x, float* out, int mode, int B, int F, int J, int C, TrainBuffers& tb, hipStream_t s,
              int accumulate = 1) {
    const int G = group_sum_groups(mode, B, F, J);
    int per;
    const int chunks = group_chunks(group_sum_count(mode, B, F, J), per);
    if ((size_t)chunks * G * C > tb.partial_floats) return fail(PAFUSE_E_WORKSPACE, "group_sum: partial buffer");
    int rc = launch<group_sum_kernel>("group_sum_kernel", dim3((unsigned)G, (unsigned)chunks), 256, 0, s, x, tb.partial, mode, B, F, J, C, G, per);
    if (rc) return rc;
    return reduce_into(tb.partial, out, G * C, chunks, (int64_t)G * C, s, accumulate);
}

// out[NI][C] (+)= sum_rows s[row][i] x[row][c]
int outer_sum(const float* sv, const float* x, float* out, int64_t M, int NI, int C, TrainBuffers& tb, hipStream_t s,
              int accumulate) {
    int64_t rows;
    const int chunks = row_chunks(M, rows);
    if ((size_t)chunks * NI * C > tb.partial_floats) return fail(PAFUSE_E_WORKSPACE, "outer_sum: partial buffer");
    int rc = launch<outer_sum_kernel>("outer_sum_kernel", (unsigned)chunks, 256, 0, s, sv, x, tb.partial, M, NI, C, rows);
    if (rc) return rc;
    return reduce_into(tb.partial, out, NI * C, chunks, (int64_t)NI * C, s, accumulate);
}

// head: out = hn Wh^T + bh (mixste.py:208-211,291).  d head_w [3,C] += dout^T hn, d head_b [3] += column sums of dout,
// dhn [M,C] = dout Wh (overwritten)
int head_grad(const float* dout, const float* hn, const float* head_w, float* d_head_w, float* d_head_b, float* dhn, int64_t M,
              int C, TrainBuffers& tb, hipStream_t s) {
    int rc;
    if ((rc = outer_sum(dout, hn, d_head_w, M, 3, C, tb, s, 1))) return rc;
    if ((rc = bias_grad(dout, d_head_b, M, 3, tb, s))) return rc;
    return launch<head_backward_kernel>("head_backward_kernel", blocks_for(M * C), 256, 0, s, dout, head_w, dhn, M, C);
}

// first layer: x0 = in5 Wpatch^T + b + pos_s[j] + temb[b] (mixste.py:222-227), g = d x0 [B*F*J,C].  d patch_w [C,5] += g^T in5
// (through the [5,C] sums in tb.small), d patch_b [C] += column sums of g, d pos_spatial [J,C] += sums per joint,
// dtemb [B,C] = sums per sample (overwritten; may be tb.small: the [5,C] sums have been read by then)
int patch_grad(const float* in5, const float* g, float* d_patch_w, float* d_patch_b, float* d_pos_spatial, float* dtemb, int B,
               int F, int J, int C, TrainBuffers& tb, hipStream_t s) {
    const int64_t M = (int64_t)B * F * J;
    int rc;
    if ((rc = outer_sum(in5, g, tb.small, M, 5, C, tb, s, 0))) return rc;
    if ((rc = launch<transpose_small_kernel>("transpose_small_kernel", blocks_for(5 * C), 256, 0, s, tb.small, d_patch_w, 5, C))) return rc;
    if ((rc = bias_grad(g, d_patch_b, M, C, tb, s))) return rc;
    if ((rc = group_sum(g, d_pos_spatial, 0, B, F, J, C, tb, s))) return rc;
    return group_sum(g, dtemb, 2, B, F, J, C, tb, s, 0);
}

template <int LP, int DP>
int launch_attn_backward_mfma(const AttnBackwardParams& ab, hipStream_t s) {
    constexpr size_t lds = ((size_t)4 * LP * (DP + 4) + 3 * LP) * sizeof(float);   // <= 47 KB
    return launch<attn_backward_mfma_kernel<LP, DP>>("attn_backward_mfma_kernel", (unsigned)(ab.nseq * ab.heads), (LP / 16) * 64, lds, s, ab);
}

template <int DP>
int launch_attn_backward_long(const AttnBackwardParams& ab, hipStream_t s) {
    constexpr size_t lds = ((size_t)2 * ATTN_BWD_LONG_LP * (DP + 4) + 3 * ATTN_BWD_LONG_LP) * sizeof(float);   // 107 KB at DP = 48
    static_assert(lds <= 160 * 1024, "LDS");
    const int64_t grid = ab.nseq * ab.heads;
    if (grid > 0x7fffffff) return fail(PAFUSE_E_ARG, "attention backward grid out of range");
    return launch<attn_backward_long_kernel<DP, 4>>("attn_backward_long_kernel", (unsigned)grid, 1024, lds, s, ab);
}

// dqkv from qkv and dO: on the fp32 matrix cores for the PAFUSE sequence lengths and head widths (L <= 80, d <= 48, d % 4 == 0),
// the FMA kernel where its two L x L planes fit the LDS, the long-sequence MFMA kernel above that (L <= 256, d <= 48)
int attention_backward(const AttnBackwardParams& ab, hipStream_t s) {
    if (ab.d % 4 == 0 && ab.d <= 48 && ab.L <= 80) {
        const int lp = ab.L <= 32 ? 32 : (ab.L <= 48 ? 48 : 80);
        if (ab.d <= 32) {
            if (lp == 32) return launch_attn_backward_mfma<32, 32>(ab, s);
            if (lp == 48) return launch_attn_backward_mfma<48, 32>(ab, s);
            return launch_attn_backward_mfma<80, 32>(ab, s);
        }
        if (lp == 32) return launch_attn_backward_mfma<32, 48>(ab, s);
        if (lp == 48) return launch_attn_backward_mfma<48, 48>(ab, s);
        return launch_attn_backward_mfma<80, 48>(ab, s);
    }
    const int L4 = (ab.L + 3) / 4 * 4;
    const size_t lds = ((size_t)4 * L4 * attn_bwd_pitch(ab.d) + (size_t)2 * ab.L * (L4 + 1)) * sizeof(float);
    if (lds > 160 * 1024 && ab.d % 4 == 0 && ab.d <= 48 && ab.L <= ATTN_BWD_LONG_LP)   // long clips: no L x L plane
        return ab.d <= 32 ? launch_attn_backward_long<32>(ab, s) : launch_attn_backward_long<48>(ab, s);
    if (lds > 160 * 1024)
        return fail(PAFUSE_E_SHAPE, "attention backward: L=%d d=%d exceed LDS (sequences of up to %d tokens at head dim <= 48)", ab.L, ab.d,
                    ATTN_BWD_LONG_LP);
    // (the ceiling is raised to the whole 160 KB once, whatever this launch's L needs)
    return launch_lds<attn_backward_kernel>("attn_backward_kernel", (unsigned)(ab.nseq * ab.heads), 256, lds, 160 * 1024, s, ab);
}

struct BlockGeometry {
    const pafuse_block_weights* w;
    bool spatial;
    int64_t nseq, group, group_stride, seq_stride, tok_stride;
    int L;
    SeqMap map;
    const float *post_w, *post_b;  // Spatial_norm / Temporal_norm
};

BlockGeometry block_geometry(const pafuse_mixste2_weights* w, int k, int64_t R) {
    const int F = w->frames, J = w->joints, i = k / 2;
    BlockGeometry g{};
    g.spatial = (k % 2) == 0;
    if (g.spatial) {
        g.w = &w->ste[i], g.nseq = R * F, g.L = J, g.group = 1, g.group_stride = J, g.seq_stride = 0, g.tok_stride = 1;
        g.map = SeqMap{0, J, F * J}, g.post_w = w->snorm_w, g.post_b = w->snorm_b;
    } else {
        g.w = &w->tte[i], g.nseq = R * J, g.L = F, g.group = J, g.group_stride = (int64_t)F * J, g.seq_stride = 1;
        g.tok_stride = J, g.map = SeqMap{1, J, F * J}, g.post_w = w->tnorm_w, g.post_b = w->tnorm_b;
    }
    return g;
}

// kind of the batch item that makes the image of W^T [K, N] for a dX GEMM: the dX GEMM's output columns are the weight's K
inline int transposed_split_kind(int K) { return plain_layout(K, false) == WLAYOUT_M16 ? 4 : 2; }

// appends weight W [N, K] (as it lies) to a split_weights_batch_kernel launch; returns the launch's workgroup count after it
int add_split_item(SplitBatchParams& p, int blocks, const float* W, uint8_t* out, int N, int K, int kind) {
    SplitBatchItem& it = p.item[p.count++];
    it.W = W, it.out = out, it.N = N, it.K = K, it.kind = kind, it.first_block = blocks;
    return blocks + (int)(((int64_t)N * (K / 8) + 255) / 256);
}

// the images of every block's four linear weights in one launch: of W for the forward (qkv, fc1 in the plain layout; proj, fc2
// in the whole-row layout), of W^T for the backward's dX GEMMs.  Sets tb.img[k][0..3] (null where the GEMM runs fp32 products).
int prepare_images(const pafuse_mixste2_weights* w, int B, bool transposed, TrainBuffers& tb, hipStream_t s) {
    const int C = w->channels, nblk = 2 * w->depth;
    const int64_t M = (int64_t)B * w->frames * w->joints;
    if (!tb.split) return PAFUSE_OK;
    SplitBatchParams p{};
    int blocks = 0;
    for (int k = 0; k < nblk; ++k) {
        const pafuse_block_weights* bw = (k % 2 == 0) ? &w->ste[k / 2] : &w->tte[k / 2];
        const float* W[4] = {bw->qkv_w, bw->proj_w, bw->fc1_w, bw->fc2_w};
        const int N[4] = {3 * C, C, 2 * C, C}, K[4] = {C, C, C, 2 * C};
        uint8_t* base = tb.wimg_blocks + (size_t)k * 48 * C * C;
        const size_t off[4] = {0, (size_t)18 * C * C, (size_t)24 * C * C, (size_t)36 * C * C};
        for (int l = 0; l < 4; ++l) {
            const bool whole_row = !transposed && (l == 1 || l == 3);
            const bool ok = transposed ? plain_splits(M, K[l], N[l]) : (whole_row ? rowln_splits(M, N[l], K[l]) : plain_splits(M, N[l], K[l]));
            tb.img[k][l] = nullptr;
            if (!ok || p.count == SPLIT_BATCH_MAX) continue;
            const int kind = transposed ? transposed_split_kind(K[l]) : (whole_row ? 1 : (plain_layout(N[l], l == 0) == WLAYOUT_M16 ? 3 : 0));
            blocks = add_split_item(p, blocks, W[l], base + off[l], N[l], K[l], kind);
            tb.img[k][l] = base + off[l];
        }
    }
    if (!p.count) return PAFUSE_OK;
    return launch<split_weights_batch_kernel>("split_weights_batch_kernel", (unsigned)blocks, 256, 0, s, p);
}

// out[B,C] = [sin(t_b freqs) | cos(t_b freqs)], freqs [C/2]: the time MLP's input
int sinusoid(const int64_t* t, const float* freqs, float* out, int B, int C, hipStream_t s) {
    return launch<sinusoid_kernel>("sinusoid_kernel", blocks_for((int64_t)B * C / 2), 256, 0, s, t, freqs, out, B, C);
}

// in5[M,5] = (x2d[M,2] | x3d[M,3]): the patch embedding's input, kept for its weight gradient
int concat_inputs(const float* x2d, const float* x3d, float* in5, int64_t M, hipStream_t s) {
    return launch<concat_inputs_kernel>("concat_inputs_kernel", blocks_for(M), 256, 0, s, x2d, x3d, in5, M);
}

int train_forward(const pafuse_mixste2_weights* w, const float* x2d, const float* x3d, const int64_t* t, int B,
                  const float* drop, float* out, TrainBuffers& tb, hipStream_t s) {
    const int F = w->frames, J = w->joints, C = w->channels, nblk = 2 * w->depth;
    const int64_t M = (int64_t)B * F * J, smax = (int64_t)B * std::max(F, J);
    int rc;
    // time MLP, unfused so that its intermediates are kept                          mixste.py:179-184,228-230
    if ((rc = sinusoid(t, w->freqs, tb.sincos, B, C, s))) return rc;
    if ((rc = plain_linear(tb.sincos, w->tm1_w, w->tm1_b, tb.uh, B, 2 * C, C, s))) return rc;
    if ((rc = gelu_fwd(tb.uh, tb.hid, (int64_t)B * 2 * C, s))) return rc;
    if ((rc = plain_linear(tb.hid, w->tm3_w, w->tm3_b, tb.temb, B, C, 2 * C, s))) return rc;
    if ((rc = concat_inputs(x2d, x3d, tb.in5, M, s))) return rc;
    EmbedParams e{};
    e.x3d = x3d, e.x2d = x2d, e.pw = w->patch_w, e.pb = w->patch_b, e.pos = w->pos_spatial, e.temb = tb.temb;
    e.n_w = w->ste[0].norm1_w, e.n_b = w->ste[0].norm1_b, e.n_eps = 1e-6f;
    e.x = tb.blk[0].x_in, e.xn = tb.blk[0].xn1;
    e.B = B, e.P = 1, e.F = F, e.J = J, e.J3 = J, e.C = C, e.nflip = 1, e.do_clamp = 0, e.scale = 1.f, e.row0 = 0, e.nrows = M;
    if ((rc = launch<embed_kernel>("embed_kernel", blocks_for(M, EMBED_ROWS_PER_BLOCK), 256, 0, s, e))) return rc;
    if ((rc = prepare_images(w, B, false, tb, s))) return rc;
    for (int k = 0; k < nblk; ++k) {
        const BlockGeometry g = block_geometry(w, k, B);
        const TrainBlockBuffers& b = tb.blk[k];
        if ((rc = plain_linear(b.xn1, g.w->qkv_w, g.w->qkv_b, b.qkv, M, 3 * C, C, s, &tb, nullptr, tb.img[k][0], true))) return rc;
        AttnParams a{};
        a.qkv = b.qkv, a.o = b.o, a.nseq = g.nseq, a.L = g.L, a.C = C, a.heads = w->heads, a.d = C / w->heads;
        a.group = g.group, a.group_stride = g.group_stride, a.seq_stride = g.seq_stride, a.tok_stride = g.tok_stride;
        a.scale = 1.0f / sqrtf((float)(C / w->heads));
        if ((rc = attention(a, s))) return rc;
        // x1 = x_in + drop * (o Wp^T + b) ; xn2 = LN2(x1): the whole-row GEMM epilogue of inference + the row factor
        GemmParams q{};
        q.A = b.o, q.W = g.w->proj_w, q.bias = g.w->proj_b, q.M = M, q.N = C, q.K = C;
        q.resid = b.x_in, q.out_x = b.x1, q.out_n = b.xn2;
        q.next_w = g.w->norm2_w, q.next_b = g.w->norm2_b, q.next_eps = 1e-6f;
        q.rowscale = drop ? drop + (int64_t)(2 * k) * smax : nullptr;
        q.rs_temporal = g.map.temporal, q.rs_J = g.map.J, q.rs_FJ = g.map.FJ;
        if ((rc = rowln_train(q, tb, s, tb.img[k][1]))) return rc;
        // u = xn2 W1^T + b1 and h = gelu(u), both kept, from one epilogue
        if ((rc = plain_linear(b.xn2, g.w->fc1_w, g.w->fc1_b, b.u, M, 2 * C, C, s, &tb, b.h, tb.img[k][2]))) return rc;
        // x2 = x1 + drop * (h W2^T + b) (kept) ; y = postLN(x2) (+ pos) -> next block's input ; its LN1 / the head
        q = GemmParams{};
        q.A = b.h, q.W = g.w->fc2_w, q.bias = g.w->fc2_b, q.M = M, q.N = C, q.K = 2 * C;
        q.resid = b.x1, q.out_pre = b.x2;
        q.rowscale = drop ? drop + (int64_t)(2 * k + 1) * smax : nullptr;
        q.rs_temporal = g.map.temporal, q.rs_J = g.map.J, q.rs_FJ = g.map.FJ;
        q.post_w = g.post_w, q.post_b = g.post_b, q.post_eps = 1e-6f;
        if (k == 0) q.pos = w->pos_temporal, q.posJ = J, q.posF = F;
        if (k + 1 < nblk) {
            const BlockGeometry n = block_geometry(w, k + 1, B);
            q.out_x = tb.blk[k + 1].x_in, q.out_n = tb.blk[k + 1].xn1;
            q.next_w = n.w->norm1_w, q.next_b = n.w->norm1_b, q.next_eps = 1e-6f;
        } else {
            q.out_x = tb.y_last, q.out_n = tb.hn, q.next_w = w->hnorm_w, q.next_b = w->hnorm_b, q.next_eps = 1e-5f;
            q.head_w = w->head_w, q.head_b = w->head_b, q.out_head = out;
        }
        if ((rc = rowln_train(q, tb, s, tb.img[k][3]))) return rc;
    }
    return PAFUSE_OK;
}


// The weight-gradient GEMMs hang off the dX chain (they only consume what it produces), so with a side stream they run
// next to it: `ready[i]` (recorded on the main stream) says operand i of the chain exists, `done[i]` (recorded on the
// side stream) says its weight gradient has been read out of it, which the chain waits for before it overwrites the
// buffer in the next stage / block.  One event per role, re-recorded every block.
struct SideLane {
    enum { FC2, FC1, PROJ, QKV, ROLES };
    hipStream_t main, side;
    hipEvent_t ready[ROLES] = {}, done[ROLES] = {};
    bool pending[ROLES] = {};
    bool on() const { return side != nullptr && side != main; }
    int open() {
        if (!on()) return PAFUSE_OK;
        for (int i = 0; i < ROLES; ++i)
            if (hipEventCreateWithFlags(&ready[i], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&done[i], hipEventDisableTiming) != hipSuccess)
                return fail(PAFUSE_E_HIP, "hipEventCreate failed");
        return PAFUSE_OK;
    }
    hipStream_t fork(int role) {  // operand of `role` is complete on the main stream: the side stream may read it
        if (!on()) return main;
        hipEventRecord(ready[role], main);
        hipStreamWaitEvent(side, ready[role], 0);
        return side;
    }
    void mark(int role) {  // the side stream has issued everything that reads the operand of `role`
        if (!on()) return;
        hipEventRecord(done[role], side);
        pending[role] = true;
    }
    void wait(int role) {  // the main stream is about to overwrite the operand of `role`
        if (!on() || !pending[role]) return;
        hipStreamWaitEvent(main, done[role], 0);
        pending[role] = false;
    }
    void close() {
        if (!on()) return;
        for (int i = 0; i < ROLES; ++i) wait(i);
        for (int i = 0; i < ROLES; ++i) {
            if (ready[i]) hipEventDestroy(ready[i]);
            if (done[i]) hipEventDestroy(done[i]);
        }
    }
};

int train_backward_blocks(const pafuse_mixste2_weights* w, const pafuse_mixste2_weights* gr, int B, const float* drop,
                          TrainBuffers& tb, hipStream_t s, SideLane& lane);

// every pointer of `gr` addresses the gradient of the like-named weight; the call ADDS into them
int train_backward(const pafuse_mixste2_weights* w, const pafuse_mixste2_weights* gr, const float* dout, int B,
                   const float* drop, TrainBuffers& tb, hipStream_t s, hipStream_t side) {
    const int F = w->frames, J = w->joints, C = w->channels;
    const int64_t M = (int64_t)B * F * J;
    auto G = [](const float* p) { return const_cast<float*>(p); };
    int rc;
    if (hipMemsetAsync(tb.zeros, 0, (size_t)3 * C * 4, s) != hipSuccess) return fail(PAFUSE_E_HIP, "memset failed");
    // head: out = LN_h(y) Wh^T + bh                                                  mixste.py:208-211,291
    if ((rc = head_grad(dout, tb.hn, w->head_w, G(gr->head_w), G(gr->head_b), tb.g2, M, C, tb, s))) return rc;
    if ((rc = ln_backward(tb.g2, tb.y_last, w->hnorm_w, 1e-5f, nullptr, tb.g, nullptr, SeqMap{}, nullptr, G(gr->hnorm_w),
                          G(gr->hnorm_b), nullptr, M, C, tb, s)))
        return rc;
    SideLane lane;
    lane.main = s, lane.side = side;
    if ((rc = lane.open())) {
        lane.close();
        return rc;
    }
    if (!(rc = prepare_images(w, B, true, tb, s))) rc = train_backward_blocks(w, gr, B, drop, tb, s, lane);
    lane.close();  // joins the side stream on every path
    if (rc) return rc;
    // x0 = in5 Wpatch^T + b + pos_s[j] + temb[b]                                     mixste.py:222-227
    float* dtemb = tb.small;  // [B,C]
    if ((rc = patch_grad(tb.in5, tb.g, G(gr->patch_w), G(gr->patch_b), G(gr->pos_spatial), dtemb, B, F, J, C, tb, s))) return rc;
    // temb = gelu(sincos W1^T + b1) W3^T + b3
    float* dhid = tb.big2;  // [B,2C]
    if ((rc = weight_grad(dtemb, tb.hid, G(gr->tm3_w), B, C, 2 * C, tb, s))) return rc;
    if ((rc = bias_grad(dtemb, G(gr->tm3_b), B, C, tb, s))) return rc;
    if ((rc = input_grad(dtemb, w->tm3_w, dhid, B, C, 2 * C, tb, s))) return rc;
    if ((rc = gelu_bwd(tb.uh, dhid, dhid, G(gr->tm1_b), B, 2 * C, tb, s))) return rc;
    return weight_grad(dhid, tb.sincos, G(gr->tm1_w), B, 2 * C, C, tb, s);
}

int train_backward_blocks(const pafuse_mixste2_weights* w, const pafuse_mixste2_weights* gr, int B, const float* drop,
                          TrainBuffers& tb, hipStream_t s, SideLane& lane) {
    const int F = w->frames, J = w->joints, C = w->channels, nblk = 2 * w->depth;
    const int64_t M = (int64_t)B * F * J, smax = (int64_t)B * std::max(F, J);
    auto G = [](const float* p) { return const_cast<float*>(p); };
    int rc;
    for (int k = nblk - 1; k >= 0; --k) {
        const BlockGeometry g = block_geometry(w, k, B);
        const pafuse_block_weights* bg = g.spatial ? &gr->ste[k / 2] : &gr->tte[k / 2];
        const TrainBlockBuffers& b = tb.blk[k];
        const float* drop_attn = drop ? drop + (int64_t)(2 * k) * smax : nullptr;
        const float* drop_mlp = drop ? drop + (int64_t)(2 * k + 1) * smax : nullptr;
        // tb.g = gradient of this block's output y (after the post norm and, for block 0, the temporal pos embed)
        if (k == 0 && (rc = group_sum(tb.g, G(gr->pos_temporal), 1, B, F, J, C, tb, s))) return rc;
        // post norm: y = LN(x2)
        lane.wait(SideLane::PROJ);  // dscaled is about to be overwritten
        if ((rc = ln_backward(tb.g, b.x2, g.post_w, 1e-6f, nullptr, tb.g2, drop_mlp, g.map, tb.dscaled,
                              G(g.spatial ? gr->snorm_w : gr->tnorm_w), G(g.spatial ? gr->snorm_b : gr->tnorm_b),
                              G(bg->fc2_b), M, C, tb, s)))
            return rc;
        // x2 = x1 + drop * (gelu(u) W2^T + b2): dscaled = d(branch output), g2 = d x2
        lane.wait(SideLane::FC1);  // big2 is about to be overwritten
        if ((rc = weight_grad(tb.dscaled, b.h, G(bg->fc2_w), M, C, 2 * C, tb, lane.fork(SideLane::FC2), lane.on()))) return rc;
        lane.mark(SideLane::FC2);
        // big2 = d u = (dscaled W2) * gelu'(u), in the dX GEMM's epilogue; fc1's bias gradient = its column sums, taken by
        // the weight-gradient kernel that stages it
        if ((rc = input_grad(tb.dscaled, g.w->fc2_w, tb.big2, M, C, 2 * C, tb, s, b.u, tb.img[k][3]))) return rc;
        if ((rc = weight_grad(tb.big2, b.xn2, G(bg->fc1_w), M, 2 * C, C, tb, lane.fork(SideLane::FC1), lane.on(), G(bg->fc1_b))))
            return rc;
        lane.mark(SideLane::FC1);
        if ((rc = input_grad(tb.big2, g.w->fc1_w, tb.e, M, 2 * C, C, tb, s, nullptr, tb.img[k][2]))) return rc;
        // xn2 = LN2(x1); x1 also feeds the residual: g = d x1, dscaled = drop * d x1
        lane.wait(SideLane::FC2);  // dscaled is about to be overwritten
        if ((rc = ln_backward(tb.e, b.x1, g.w->norm2_w, 1e-6f, tb.g2, tb.g, drop_attn, g.map, tb.dscaled, G(bg->norm2_w),
                              G(bg->norm2_b), G(bg->proj_b), M, C, tb, s)))
            return rc;
        // x1 = x_in + drop * (o Wp^T + bp)
        if ((rc = weight_grad(tb.dscaled, b.o, G(bg->proj_w), M, C, C, tb, lane.fork(SideLane::PROJ), lane.on()))) return rc;
        lane.mark(SideLane::PROJ);
        if ((rc = input_grad(tb.dscaled, g.w->proj_w, tb.e, M, C, C, tb, s, nullptr, tb.img[k][1]))) return rc;
        lane.wait(SideLane::QKV);  // big1 is about to be overwritten
        AttnBackwardParams ab{};
        ab.qkv = b.qkv, ab.d_o = tb.e, ab.dqkv = tb.big1, ab.nseq = g.nseq, ab.group = g.group;
        ab.group_stride = g.group_stride, ab.seq_stride = g.seq_stride, ab.tok_stride = g.tok_stride;
        ab.L = g.L, ab.C = C, ab.heads = w->heads, ab.d = C / w->heads, ab.scale = 1.0f / sqrtf((float)(C / w->heads));
        if ((rc = attention_backward(ab, s))) return rc;
        {
            hipStream_t ss = lane.fork(SideLane::QKV);
            if ((rc = weight_grad(tb.big1, b.xn1, G(bg->qkv_w), M, 3 * C, C, tb, ss, lane.on(), G(bg->qkv_b)))) return rc;
            lane.mark(SideLane::QKV);
        }
        if ((rc = input_grad(tb.big1, g.w->qkv_w, tb.e, M, 3 * C, C, tb, s, nullptr, tb.img[k][0]))) return rc;
        // xn1 = LN1(x_in); x_in also feeds the residual: g <- d x_in (in place: add and dx are the same element)
        if ((rc = ln_backward(tb.e, b.x_in, g.w->norm1_w, 1e-6f, tb.g, tb.g, nullptr, SeqMap{}, nullptr, G(bg->norm1_w),
                              G(bg->norm1_b), nullptr, M, C, tb, s)))
            return rc;
    }
    return PAFUSE_OK;
}

