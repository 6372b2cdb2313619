// lg_learner.hip -- fused actor and PPO learner: the lg_policy_*, lg_mlp_*, lg_mlp_wide_*, lg_ppo_*, lg_adam_step, lg_gae_returns and
// lg_rollout_record / lg_rollout_finish entry points of include/legged_hip.h, with the kernels of lg_policy.h (and its two non-template pack
// kernels), lg_train.h and lg_gemm.h.  Nothing here touches an lg_sim handle.  One actor, k_policy_act<3,8,4,2>, is launched from
// lg_kernels.hip (launch_policy_act_flat, lg_host.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <new>

#include "lg_host.h"                 // with lg_device.h and lg_policy.h
#include "lg_dec_game_common.h"      // launchers of lg_dec_game.hip (declarations only)
#include "lg_train.h"
#include "lg_gemm.h"

using namespace lg;

// ------------------------------------------------------------------ fused actor (lg_policy.h): host side
static int g_wide_precision = 1;       /* lg_mlp_wide_set_precision: 0 = f32 MFMA kernels, 1 = split-bf16 (bf16x3) kernels, learner GEMMs and wide actor alike */
int lg::wide_precision() { return g_wide_precision; }
void lg::fill_policy_args(const lg_policy *p, PolicyArgs &a, const float *obs, float *actions, float *mean, int32_t num_envs, uint64_t seed,
                          int64_t step, const int64_t *step_counter, int32_t deterministic) {
    a.obs = obs; a.actions = actions; a.mean = mean; a.std = p->d_std; a.step_counter = step_counter; a.step = step; a.seed = seed;
    a.num_envs = num_envs; a.num_obs = p->dims[0]; a.num_actions = p->dims[4]; a.deterministic = deterministic;
    for (int i = 0; i < 4; i++) { a.w[i] = p->d_w[i]; a.b[i] = p->d_b[i]; }
}
void lg::fill_wide_operands(const lg_policy *p, const lg::bf16x8g *(&wb)[4], const float *(&bb)[4]) {
    for (int i = 0; i < 4; i++) { wb[i] = reinterpret_cast<const lg::bf16x8g *>(p->d_wb[i]); bb[i] = p->d_bb[i]; }
}
// torch Linear [out,in] -> MFMA A-operand stream [out_tile][k_step = (t,r)][lane]: W[16o + (l&15)][16t + 4(l>>4) + r]
static void policy_pack_layer(const float *W, const float *bias, int in_dim, int out_dim, int in_tiles, int out_tiles,
                              float *w_packed, float *b_packed) {
    for (int o = 0; o < out_tiles; o++) {
        for (int t = 0; t < in_tiles; t++) for (int r = 0; r < 4; r++) for (int l = 0; l < 64; l++) {
            int row = 16 * o + (l & 15), col = 16 * t + 4 * (l >> 4) + r;
            w_packed[((size_t)(o * in_tiles + t) * 4 + r) * 64 + l] = (row < out_dim && col < in_dim) ? W[(size_t)row * in_dim + col] : 0.0f;
        }
        for (int r = 0; r < 4; r++) for (int l = 0; l < 64; l++) {       // D layout: lane l, reg r = row 16o + 4(l>>4) + r
            int row = 16 * o + 4 * (l >> 4) + r;
            b_packed[(o * 4 + r) * 64 + l] = row < out_dim ? bias[row] : 0.0f;
        }
    }
}

// device version of policy_pack_layer: one thread per packed element
__global__ void k_policy_pack(const float *__restrict__ W, const float *__restrict__ bias, int in_dim, int out_dim, int in_tiles, int out_tiles,
                              float *__restrict__ w_packed, float *__restrict__ b_packed) {
    const size_t nw = (size_t)out_tiles * in_tiles * 4 * 64, nb = (size_t)out_tiles * 4 * 64;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nw + nb; i += (size_t)gridDim.x * blockDim.x) {
        if (i < nw) {
            const int l = (int)(i & 63), r = (int)((i >> 6) & 3);
            const size_t ot = i >> 8;
            const int t = (int)(ot % in_tiles), o = (int)(ot / in_tiles);
            const int row = 16 * o + (l & 15), col = 16 * t + 4 * (l >> 4) + r;
            w_packed[i] = (row < out_dim && col < in_dim) ? W[(size_t)row * in_dim + col] : 0.0f;
        } else {
            const size_t j = i - nw;
            const int l = (int)(j & 63), r = (int)((j >> 6) & 3), o = (int)(j >> 8);
            const int row = 16 * o + 4 * (l >> 4) + r;
            b_packed[j] = row < out_dim ? bias[row] : 0.0f;
        }
    }
}

// ---- PPO learner: MLP forward / backward for up to two nets (actor, critic) in one launch -------------------------------------
#define LG_TRAIN_WGS 256           /* workgroups per net = partial-sum slices */
static unsigned long long *g_mlp_trace = nullptr;   /* diagnostic, see lg_mlp_trace */
#define LG_FWD_SLOTS 4             /* row tiles in flight per workgroup (forward: 140 KB of LDS) */
#define LG_BWD_SLOTS 2             /* backward: 152 KB */
static int mlp_fill(const lg_mlp_net *nets, int32_t n_nets, const int64_t *rows, int32_t mb, lg::MlpArgs &a, int &wgs, int slots, bool partials) {
    if (!nets || n_nets < 1 || n_nets > 2 || mb <= 0) return fail(-1, "bad argument");
    memset(&a, 0, sizeof a);
    a.rows = rows; a.mb = mb; a.n_tiles = (mb + 15) / 16; a.trace = g_mlp_trace;
    // persistent workgroups, one per CU (the LDS-resident weights allow no more): the CUs are split between the nets
    static int num_cus = 0;
    if (!num_cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || num_cus <= 0)
            num_cus = 256;
    }
    wgs = num_cus / n_nets;
    if (partials && wgs > LG_TRAIN_WGS) wgs = LG_TRAIN_WGS;                       // backward: one partial-sum slice per workgroup
    if (wgs * slots > a.n_tiles) wgs = (a.n_tiles + slots - 1) / slots;
    if (wgs < 1) wgs = 1;
    for (int n = 0; n < n_nets; n++) {
        const lg_mlp_net &s = nets[n];
        lg::MlpNetArgs &d = a.net[n];
        if (!s.input) return fail(-1, "null input");
        if (s.dims[0] <= 0 || s.dims[0] > 48 || s.dims[1] != 128 || s.dims[2] != 64 || s.dims[3] != 32 || s.dims[4] <= 0 || s.dims[4] > 16)
            return fail(-4, "lg_mlp_*: only the <=48-128-64-32-<=16 MLP shape is built");
        int gf = 0;
        for (int l = 0; l < 4; l++) {
            if (!s.weights[l] || !s.biases[l]) return fail(-1, "null layer pointer");
            if (l > 0 && ((uintptr_t)s.weights[l] & 15)) return fail(-4, "weights must be 16-byte aligned");
            d.w[l] = s.weights[l]; d.b[l] = s.biases[l];
            gf += s.dims[l + 1] * s.dims[l] + s.dims[l + 1];
        }
        d.x = s.input; d.y = s.output; d.dy = s.grad_output; d.grad_floats = gf; d.part_stride = gf + LG_PPO_EXTRA;
        memcpy(d.dims, s.dims, sizeof d.dims);
    }
    return 0;
}

extern "C" {

/* diagnostic (tools/mlp_probe.py): later lg_mlp_* launches write up to 60 s_memtime stamps of workgroup (0,0) to `buf` (device, u64[60]); null stops */
void lg_mlp_trace(unsigned long long *buf) { g_mlp_trace = buf; }

int lg_mlp_forward(const lg_mlp_net *nets, int32_t n_nets, const int64_t *rows, int32_t mb, void *stream) {
    lg::MlpArgs a; int wgs;
    if (int rc = mlp_fill(nets, n_nets, rows, mb, a, wgs, LG_FWD_SLOTS, false)) return rc;
    for (int n = 0; n < n_nets; n++) if (!nets[n].output) return fail(-1, "null output");
    constexpr size_t lds_bytes = lg::TrainLds<3, 8, 4, 2, false, LG_FWD_SLOTS>::floats * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void *)lg::k_mlp_train<3, 8, 4, 2, false, LG_FWD_SLOTS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        attr_set = true;
    }
    hipLaunchKernelGGL((lg::k_mlp_train<3, 8, 4, 2, false, LG_FWD_SLOTS>), dim3(wgs, n_nets), dim3(64 * LG_TRAIN_WAVES * LG_FWD_SLOTS), lds_bytes, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t lg_mlp_workspace_bytes(const lg_mlp_net *nets, int32_t n_nets) {
    size_t total = 0;
    if (!nets) return 0;
    for (int n = 0; n < n_nets; n++) {
        size_t gf = 0;
        for (int l = 0; l < 4; l++) gf += (size_t)nets[n].dims[l + 1] * nets[n].dims[l] + nets[n].dims[l + 1];
        total += (gf + LG_PPO_EXTRA) * LG_TRAIN_WGS * sizeof(float);
    }
    return total;
}

// shared by lg_mlp_backward (batch == null: dL/dy from nets[n].grad_output) and lg_ppo_minibatch (dL/dy from the fused PPO loss)
static int mlp_backward_launch(const lg_mlp_net *nets, int32_t n_nets, const int64_t *rows, int32_t mb, const lg_ppo_batch *batch,
                               float *workspace, size_t workspace_bytes, void *stream) {
    lg::MlpArgs a; int wgs;
    if (int rc = mlp_fill(nets, n_nets, rows, mb, a, wgs, LG_BWD_SLOTS, true)) return rc;
    if (!workspace || workspace_bytes < lg_mlp_workspace_bytes(nets, n_nets)) return fail(-1, "workspace too small (lg_mlp_workspace_bytes)");
    lg::MlpReduceArgs r; memset(&r, 0, sizeof r);
    float *ws = workspace;
    int max_gf = 0;
    for (int n = 0; n < n_nets; n++) {
        if (!batch && !nets[n].grad_output) return fail(-1, "null grad_output");
        a.net[n].partial = ws; r.partial[n] = ws; ws += (size_t)a.net[n].part_stride * LG_TRAIN_WGS;
        r.grad_floats[n] = a.net[n].grad_floats; r.part_stride[n] = a.net[n].part_stride;
        if (a.net[n].grad_floats > max_gf) max_gf = a.net[n].grad_floats;
        memcpy(r.dims[n], nets[n].dims, sizeof r.dims[n]);
        for (int l = 0; l < 4; l++) {
            if (!nets[n].grad_weights[l] || !nets[n].grad_biases[l]) return fail(-1, "null gradient pointer");
            r.gw[n][l] = nets[n].grad_weights[l]; r.gb[n][l] = nets[n].grad_biases[l];
        }
    }
    r.n_partials = wgs;                        // the groups of a workgroup fold their sums before writing
    if (batch) {
        if (n_nets != 2 || nets[1].dims[4] != 1) return fail(-1, "lg_ppo_minibatch needs nets = {actor, critic (one output)}");
        if (!rows || !batch->actions || !batch->old_log_prob || !batch->old_mu || !batch->old_sigma || !batch->advantages || !batch->old_values ||
            !batch->returns || !batch->std || !batch->d_std || !batch->stats) return fail(-1, "null PPO batch pointer");
        a.ppo = lg::PpoArgs{batch->actions, batch->old_log_prob, batch->old_mu, batch->old_sigma, batch->advantages, batch->old_values, batch->returns,
                            batch->std, batch->clip, batch->value_coef, 1.0f / (float)mb, batch->use_clipped_value};
        r.loss = 1; r.num_actions = nets[0].dims[4]; r.std = batch->std; r.ecoef = batch->entropy_coef; r.d_std = batch->d_std; r.stats = batch->stats; r.loss_acc = batch->loss_acc;
    }
    hipStream_t st = (hipStream_t)stream;
    constexpr size_t lds_bytes = lg::TrainLds<3, 8, 4, 2, true, LG_BWD_SLOTS>::floats * sizeof(float);
    static_assert(lds_bytes <= 160 * 1024, "k_mlp_train backward exceeds the CU's LDS");
    static bool attr_set = false;
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void *)lg::k_mlp_train<3, 8, 4, 2, true, LG_BWD_SLOTS, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        HIP_TRY(hipFuncSetAttribute((const void *)lg::k_mlp_train<3, 8, 4, 2, true, LG_BWD_SLOTS, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        attr_set = true;
    }
    if (batch) hipLaunchKernelGGL((lg::k_mlp_train<3, 8, 4, 2, true, LG_BWD_SLOTS, true>), dim3(wgs, n_nets), dim3(64 * LG_TRAIN_WAVES * LG_BWD_SLOTS), lds_bytes, st, a);
    else hipLaunchKernelGGL((lg::k_mlp_train<3, 8, 4, 2, true, LG_BWD_SLOTS, false>), dim3(wgs, n_nets), dim3(64 * LG_TRAIN_WAVES * LG_BWD_SLOTS), lds_bytes, st, a);
    hipLaunchKernelGGL(lg::k_mlp_reduce, dim3((max_gf + (batch ? LG_PPO_EXTRA : 0) + 31) / 32, n_nets), dim3(256), 0, st, r);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_mlp_backward(const lg_mlp_net *nets, int32_t n_nets, const int64_t *rows, int32_t mb, float *workspace, size_t workspace_bytes,
                    void *stream) {
    return mlp_backward_launch(nets, n_nets, rows, mb, nullptr, workspace, workspace_bytes, stream);
}

int lg_ppo_minibatch(const lg_mlp_net *nets, const int64_t *rows, int32_t mb, const lg_ppo_batch *batch, float *workspace,
                     size_t workspace_bytes, void *stream) {
    if (!batch) return fail(-1, "null batch");
    return mlp_backward_launch(nets, 2, rows, mb, batch, workspace, workspace_bytes, stream);
}

// ---- learner kernels for the wide MLPs (lg_gemm.h): per layer a tiled f32-MFMA GEMM with the element-wise work in its epilogue
struct WideLayout { size_t x[4], g[4], part[4], x0p, w0p, wpk[4], bpk[4], total; int splits[4]; int kchunk[4]; int k0p; int ks[4], ot[4]; bool chain; int out_chunks; bool out_narrow; };      // float offsets into one net's workspace slice
static void wide_layout(const lg_mlp_net &n, int mb, WideLayout &L) {
    size_t o = 0;
    for (int l = 1; l <= 3; l++) { L.x[l] = o; o += (size_t)mb * n.dims[l]; }
    for (int l = 1; l <= 3; l++) { L.g[l] = o; o += (size_t)mb * n.dims[l]; }
    L.out_narrow = n.dims[3] == 128 && n.dims[4] <= LG_OUT_MAXN;      // k_wide_out_bwd: dX + dW of the output layer in one pass
    L.out_chunks = mb >= 2048 ? 256 : (mb + 7) / 8;
    o = (o + 3) & ~(size_t)3;
    for (int l = 0; l < 4; l++) {                                     // one partial buffer per layer: all four are summed by ONE k_wide_reduce launch
        const int tiles = ((n.dims[l + 1] + LG_GT - 1) / LG_GT) * ((n.dims[l] + LG_GT - 1) / LG_GT);
        int sp = (384 + tiles - 1) / tiles;                                   // enough workgroups for the chip: tiles x splits >= ~1.5 x CUs
        if (sp > LG_WIDE_MAX_SPLITS) sp = LG_WIDE_MAX_SPLITS;
        int chunk = (mb + sp - 1) / sp;
        chunk = ((chunk + LG_BK - 1) / LG_BK) * LG_BK;       /* multiple of both kernels' stage depths */
        if (chunk < LG_BK) chunk = LG_BK;
        sp = (mb + chunk - 1) / chunk;
        L.splits[l] = sp; L.kchunk[l] = chunk;
        size_t p = (size_t)sp * n.dims[l + 1] * ((n.dims[l] + 1 + 3) & ~3);
        if (l == 3 && L.out_narrow) { const size_t q = (size_t)L.out_chunks * n.dims[4] * ((n.dims[3] + 1 + 3) & ~3); if (q > p) p = q; }
        L.part[l] = o; o += (p + 3) & ~(size_t)3;
    }
    L.k0p = (n.dims[0] + 3) & ~3;                     // aligned, gather-free copies of the layer-0 operands (k_wide_prep)
    L.x0p = o; o += (size_t)mb * L.k0p;
    L.w0p = o; o += (size_t)n.dims[1] * L.k0p;
    // chain forward (k_mlp_chain_fwd64): split-bf16 operand streams of the four layers, re-packed every call
    const int k0s = (n.dims[0] + 15) / 16;
    L.chain = n.dims[1] == 512 && n.dims[2] == 256 && n.dims[3] == 128 && n.dims[4] <= 16 && (k0s == 15 || k0s == 11);
    for (int l = 0; l < 4; l++) {
        L.ks[l] = l == 0 ? k0s : n.dims[l] / 16; L.ot[l] = (n.dims[l + 1] + 31) / 32;
        o = (o + 3) & ~(size_t)3;
        L.wpk[l] = o; if (L.chain) o += (size_t)L.ot[l] * L.ks[l] * 512;          // 1024 bf16 per (tile, k-step)
        L.bpk[l] = o; if (L.chain) o += (size_t)L.ot[l] * 32;
    }
    L.total = (o + 3) & ~(size_t)3;
}
// The gathered, padded copy of net n's input rows (k_wide_prep).  Actor and critic of the registered tasks read the SAME observation
// tensor (no privileged observations): one copy then serves both nets -- half the gather traffic, and layer 0's dW / the chain forward
// of the second net find the rows in cache.
static bool wide_shared_input(const lg_mlp_net *nets, int32_t n_nets) {
    return n_nets == 2 && nets[0].input == nets[1].input && nets[0].dims[0] == nets[1].dims[0];
}
static float *wide_x0p(const lg_mlp_net *nets, int32_t n_nets, int32_t mb, float *workspace, int n) {
    float *ws = workspace;
    const int owner = wide_shared_input(nets, n_nets) ? 0 : n;
    for (int i = 0; i < owner; i++) { WideLayout L; wide_layout(nets[i], mb, L); ws += L.total; }
    WideLayout L; wide_layout(nets[owner], mb, L);
    return ws + L.x0p;
}
static int wide_check(const lg_mlp_net *nets, int32_t n_nets, int32_t mb) {
    if (!nets || n_nets < 1 || n_nets > 2 || mb <= 0) return fail(-1, "bad argument");
    for (int n = 0; n < n_nets; n++) {
        for (int l = 0; l <= 4; l++) if (nets[n].dims[l] <= 0 || nets[n].dims[l] > 4096) return fail(-4, "lg_mlp_wide_*: layer widths must be in 1..4096");
        for (int l = 0; l < 4; l++) if (!nets[n].weights[l] || !nets[n].biases[l]) return fail(-1, "null layer pointer");
        if (!nets[n].input) return fail(-1, "null input");
    }
    return 0;
}

/* g_wide_precision (defined with the fused-actor host code): 0: exact f32 MFMA (k_gemm_wide), 1: split-bf16 (k_gemm_wide_bf16x3) */
#define LAUNCH_WIDE(MODE, GRID, ARGS)                                                                              \
    { if (g_wide_precision == 0) hipLaunchKernelGGL((lg::k_gemm_wide<MODE>), GRID, dim3(256), 0, st, ARGS);       \
      else hipLaunchKernelGGL((lg::k_gemm_wide_bf16x3<MODE>), GRID, dim3(256), 0, st, ARGS); }

/* 0: exact f32 MFMA; 1 (default): split-bf16 products hi*hi + hi*lo + lo*hi with f32 accumulation (~2^-15 relative, ~5 x faster).  Returns the previous setting. */
int lg_mlp_wide_set_precision(int mode) { const int old = g_wide_precision; if (mode == 0 || mode == 1) g_wide_precision = mode; return old; }

size_t lg_mlp_wide_workspace_bytes(const lg_mlp_net *nets, int32_t n_nets, int32_t mb) {
    if (!nets || mb <= 0) return 0;
    size_t total = 0;
    for (int n = 0; n < n_nets; n++) { WideLayout L; wide_layout(nets[n], mb, L); total += L.total; }
    return total * sizeof(float);
}

int lg_mlp_wide_forward(const lg_mlp_net *nets, int32_t n_nets, const int64_t *rows, int32_t mb, float *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = wide_check(nets, n_nets, mb)) return rc;
    if (!workspace || workspace_bytes < lg_mlp_wide_workspace_bytes(nets, n_nets, mb)) return fail(-1, "workspace too small (lg_mlp_wide_workspace_bytes)");
    for (int n = 0; n < n_nets; n++) if (!nets[n].output) return fail(-1, "null output");
    hipStream_t st = (hipStream_t)stream;
    {   // layer-0 operands: gathered, padded, aligned
        lg::WidePrepArgs pr; memset(&pr, 0, sizeof pr);
        float *ws = workspace;
        size_t work = 0;
        for (int n = 0; n < n_nets; n++) {
            WideLayout L; wide_layout(nets[n], mb, L);
            pr.x[n] = nets[n].input; pr.w[n] = nets[n].weights[0]; pr.xp[n] = ws + L.x0p; pr.wp[n] = ws + L.w0p;
            pr.skip_x[n] = n > 0 && wide_shared_input(nets, n_nets);
            pr.d0[n] = nets[n].dims[0]; pr.d1[n] = nets[n].dims[1]; pr.k0p[n] = L.k0p;
            const size_t w_ = ((size_t)mb + nets[n].dims[1]) * (L.k0p / 4);
            if (w_ > work) work = w_;
            ws += L.total;
        }
        pr.rows = rows; pr.mb = mb;
        int blocks = (int)((work + 255) / 256); if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(lg::k_wide_prep, dim3(blocks, n_nets), dim3(256), 0, st, pr);
    }
    bool chain = g_wide_precision == 1;
    int k0s = 0;
    for (int n = 0; n < n_nets; n++) {
        WideLayout L; wide_layout(nets[n], mb, L);
        chain = chain && L.chain && (n == 0 || L.ks[0] == k0s);
        k0s = L.ks[0];
    }
    if (chain) {                                       // all four layers in one launch, activations on chip (lg_policy.h: k_mlp_chain_fwd64)
        lg::ChainPackArgs pk; memset(&pk, 0, sizeof pk);
        lg::ChainArgs c; memset(&c, 0, sizeof c);
        c.mb = mb;
        float *ws = workspace;
        size_t work = 0;
        for (int n = 0; n < 2; n++) {
            const int m = n < n_nets ? n : 0;          // a single net: the second descriptor mirrors the first (never launched: grid z / y = n_nets)
            if (n == n_nets) ws = workspace;
            WideLayout L; wide_layout(nets[m], mb, L);
            lg::ChainNet &cn = c.net[n];
            cn.x = wide_x0p(nets, n_nets, mb, workspace, m); cn.ldx = L.k0p; cn.num_in = nets[m].dims[0];
            for (int l = 0; l < 4; l++) {
                pk.W[n][l] = nets[m].weights[l]; pk.b[n][l] = nets[m].biases[l];
                pk.wp[n][l] = reinterpret_cast<__bf16 *>(ws + L.wpk[l]); pk.bp[n][l] = ws + L.bpk[l];
                pk.in_dim[n][l] = nets[m].dims[l]; pk.out_dim[n][l] = nets[m].dims[l + 1]; pk.KS[n][l] = L.ks[l]; pk.OT[n][l] = L.ot[l];
                cn.wb[l] = reinterpret_cast<const lg::bf16x8g *>(ws + L.wpk[l]); cn.bb[l] = ws + L.bpk[l];
                const size_t w_ = (size_t)L.ot[l] * L.ks[l] * 512 + (size_t)L.ot[l] * 32;
                if (w_ > work) work = w_;
            }
            for (int l = 0; l < 3; l++) { cn.act[l] = ws + L.x[l + 1]; cn.lda[l] = nets[m].dims[l + 1]; }
            cn.out = nets[m].output; cn.out_dim = nets[m].dims[4];
            ws += L.total;
        }
        int blocks = (int)((work + 255) / 256); if (blocks > 512) blocks = 512;
        hipLaunchKernelGGL(lg::k_chain_pack, dim3(blocks, 4, n_nets), dim3(256), 0, st, pk);
        const dim3 grid((mb + 63) / 64, n_nets), block(64 * LG_PW_WAVES);                  // 64 rows per workgroup (k_mlp_chain_fwd64)
        if (k0s == 15) hipLaunchKernelGGL((lg::k_mlp_chain_fwd64<15>), grid, block, 0, st, c);
        else hipLaunchKernelGGL((lg::k_mlp_chain_fwd64<11>), grid, block, 0, st, c);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    for (int l = 0; l < 4; l++) {
        lg::GemmArgs a; memset(&a, 0, sizeof a);
        a.rows = nullptr; a.gather_a_rows = 0; a.mb = mb;
        int gx = 0, gy = 0;
        float *ws = workspace;
        for (int n = 0; n < n_nets; n++) {
            WideLayout L; wide_layout(nets[n], mb, L);
            lg::GemmNet &g = a.net[n];
            const int32_t *d = nets[n].dims;
            g.A = l == 0 ? wide_x0p(nets, n_nets, mb, workspace, n) : ws + L.x[l]; g.lda = l == 0 ? L.k0p : d[l];
            g.B = l == 0 ? ws + L.w0p : nets[n].weights[l]; g.ldb = l == 0 ? L.k0p : d[l]; g.bias = nets[n].biases[l];
            g.C = l == 3 ? nets[n].output : ws + L.x[l + 1]; g.ldc = d[l + 1];
            g.M = mb; g.N = d[l + 1]; g.K = d[l]; g.elu = l < 3; g.splits = 1; g.k_chunk = g.K;
            g.tiles_m = (g.M + LG_GT - 1) / LG_GT; g.tiles_n = (g.N + LG_GT - 1) / LG_GT;
            if (g.tiles_m > gx) gx = g.tiles_m;
            if (g.tiles_n > gy) gy = g.tiles_n;
            ws += L.total;
        }
        LAUNCH_WIDE(lg::GEMM_FWD, dim3(gx, gy, n_nets), a)
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

/* Gradients of all weights / biases given dL/d output (nets[n].grad_output); uses the activations the preceding
 * lg_mlp_wide_forward left in the same workspace. */
int lg_mlp_wide_backward(const lg_mlp_net *nets, int32_t n_nets, const int64_t *rows, int32_t mb, float *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = wide_check(nets, n_nets, mb)) return rc;
    if (!workspace || workspace_bytes < lg_mlp_wide_workspace_bytes(nets, n_nets, mb)) return fail(-1, "workspace too small (lg_mlp_wide_workspace_bytes)");
    for (int n = 0; n < n_nets; n++) {
        if (!nets[n].grad_output) return fail(-1, "null grad_output");
        for (int l = 0; l < 4; l++) if (!nets[n].grad_weights[l] || !nets[n].grad_biases[l]) return fail(-1, "null gradient pointer");
    }
    hipStream_t st = (hipStream_t)stream;
    bool narrow = true;
    for (int n = 0; n < n_nets; n++) { WideLayout L; wide_layout(nets[n], mb, L); narrow = narrow && L.out_narrow; }
    lg::WideReduceArgs red; memset(&red, 0, sizeof red);            // the partials of all layers, summed by one launch behind the last GEMM
    int red_max = 0;
    auto add_job = [&](int l, int n, const float *part, int N_, int K_, int ld, int splits, int group) {
        lg::WideReduceJob &j = red.job[2 * l + n];
        j.part = part; j.gw = nets[n].grad_weights[l]; j.gb = nets[n].grad_biases[l]; j.N = N_; j.K = K_; j.ld = ld; j.splits = splits; j.group = group;
        if (N_ * ld * group > red_max) red_max = N_ * ld * group;
    };
    for (int l = 3; l >= 0; l--) {
        if (l == 3 && narrow) {                        // the <= 16-wide output layer: G_3, dW_3, db_3 from one read of A_3 (lg_gemm.h: k_wide_out_bwd)
            lg::OutBwdArgs o; memset(&o, 0, sizeof o);
            o.mb = mb;
            int chunks = 0;
            float *ws = workspace;
            for (int n = 0; n < n_nets; n++) {
                WideLayout L; wide_layout(nets[n], mb, L);
                const int32_t *d = nets[n].dims;
                lg::OutBwdNet &q = o.net[n];
                q.dz = nets[n].grad_output; q.w = nets[n].weights[3]; q.act = ws + L.x[3]; q.g = ws + L.g[3]; q.part = ws + L.part[3];
                q.N = d[4]; q.K = d[3]; q.ld = (d[3] + 1 + 3) & ~3; q.chunks = L.out_chunks; q.rows_per_chunk = (mb + L.out_chunks - 1) / L.out_chunks;
                if (q.chunks > chunks) chunks = q.chunks;
                add_job(3, n, q.part, d[4], d[3], q.ld, q.chunks, 8);
                ws += L.total;
            }
            hipLaunchKernelGGL((lg::k_wide_out_bwd<LG_OUT_MAXN>), dim3(chunks, n_nets), dim3(256), 0, st, o);
            continue;
        }
        // dW_l, db_l (split over the mini-batch rows) ...
        lg::GemmArgs a; memset(&a, 0, sizeof a);
        a.rows = nullptr; a.gather_b_k = 0; a.mb = mb;          // layer 0 reads the gathered copy the forward pass left in the workspace
        int gx = 0, gy = 0;
        float *ws = workspace;
        for (int n = 0; n < n_nets; n++) {
            WideLayout L; wide_layout(nets[n], mb, L);
            lg::GemmNet &g = a.net[n];
            const int32_t *d = nets[n].dims;
            g.A = l == 3 ? nets[n].grad_output : ws + L.g[l + 1]; g.lda = d[l + 1];
            g.B = l == 0 ? wide_x0p(nets, n_nets, mb, workspace, n) : ws + L.x[l]; g.ldb = l == 0 ? L.k0p : d[l];
            g.C = ws + L.part[l]; g.ldc = (d[l] + 1 + 3) & ~3;
            g.M = d[l + 1]; g.N = d[l]; g.K = mb; g.splits = L.splits[l]; g.k_chunk = L.kchunk[l];
            g.tiles_m = (g.M + LG_GT - 1) / LG_GT; g.tiles_n = (d[l] + LG_GT - 1) / LG_GT;
            if (g.tiles_m > gx) gx = g.tiles_m;
            if (g.tiles_n * g.splits > gy) gy = g.tiles_n * g.splits;
            add_job(l, n, ws + L.part[l], d[l + 1], d[l], (d[l] + 1 + 3) & ~3, L.splits[l], 1);
            ws += L.total;
        }
        LAUNCH_WIDE(lg::GEMM_DW, dim3(gx, gy, n_nets), a)
        if (l == 0) break;
        // ... and G_l = (G_{l+1} W_l) * elu'(X_l)
        lg::GemmArgs b; memset(&b, 0, sizeof b);
        b.mb = mb;
        gx = gy = 0; ws = workspace;
        for (int n = 0; n < n_nets; n++) {
            WideLayout L; wide_layout(nets[n], mb, L);
            lg::GemmNet &g = b.net[n];
            const int32_t *d = nets[n].dims;
            g.A = l == 3 ? nets[n].grad_output : ws + L.g[l + 1]; g.lda = d[l + 1];
            g.B = nets[n].weights[l]; g.ldb = d[l];
            g.C = ws + L.g[l]; g.ldc = d[l]; g.act = ws + L.x[l];
            g.M = mb; g.N = d[l]; g.K = d[l + 1]; g.splits = 1; g.k_chunk = g.K;
            g.tiles_m = (g.M + LG_GT - 1) / LG_GT; g.tiles_n = (g.N + LG_GT - 1) / LG_GT;
            if (g.tiles_m > gx) gx = g.tiles_m;
            if (g.tiles_n > gy) gy = g.tiles_n;
            ws += L.total;
        }
        LAUNCH_WIDE(lg::GEMM_DX, dim3(gx, gy, n_nets), b)
    }
    hipLaunchKernelGGL(lg::k_wide_reduce, dim3((red_max + 255) / 256, LG_REDUCE_JOBS), dim3(256), 0, st, red);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_rollout_record(const lg_rollout_step *s, void *stream) {
    if (!s || !s->obs || !s->actions || !s->mean || !s->rewards || !s->dones || !s->storage_obs || !s->storage_actions || !s->storage_mu ||
        !s->storage_rewards || !s->storage_dones) return fail(-1, "null argument");
    if (s->num_envs <= 0 || s->num_obs <= 0 || s->num_actions <= 0 || s->num_actions > s->num_obs) return fail(-1, "bad sizes");
    if ((s->cur_return != nullptr) != (s->cur_length != nullptr) || (s->cur_return && !s->sums)) return fail(-1, "incomplete episode statistics");
    lg::RecordArgs a{s->obs, s->actions, s->mean, s->rewards, s->dones, s->time_outs, s->storage_obs, s->storage_actions, s->storage_mu,
                     s->storage_rewards, s->storage_dones, s->storage_time_outs, s->cur_return, s->cur_length, s->sums,
                     s->std, s->storage_sigma, s->storage_log_prob, s->num_envs, s->num_obs, s->num_actions};
    if (s->std && (!s->storage_sigma || !s->storage_log_prob)) return fail(-1, "std given without storage_sigma / storage_log_prob");
    const int64_t n = (int64_t)s->num_envs * s->num_obs;
    if (s->num_actions > 16) return fail(-1, "lg_rollout_record: at most 16 actions");
    hipLaunchKernelGGL(lg::k_rollout_record, dim3((unsigned)((n + 255) / 256 + ((int64_t)s->num_envs * 16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_rollout_finish(const lg_rollout_post *s, void *stream) {
    if (!s || !s->actions || !s->mean || !s->rewards || !s->dones || !s->std || !s->sigma || !s->log_prob) return fail(-1, "null argument");
    if (s->steps <= 0 || s->num_envs <= 0 || s->num_actions <= 0 || s->num_actions > 16) return fail(-1, "bad sizes (at most 16 actions)");
    if ((s->cur_return != nullptr) != (s->cur_length != nullptr) || (s->cur_return && !s->sums)) return fail(-1, "incomplete episode statistics");
    lg::RollPostArgs a{s->actions, s->mean, s->rewards, s->dones, s->time_outs, s->std, s->sigma, s->log_prob, s->time_outs_f,
                       s->cur_return, s->cur_length, s->sums, s->steps, s->num_envs, s->num_actions};
    const int64_t n_tr = (int64_t)s->steps * s->num_envs;
    hipLaunchKernelGGL(lg::k_rollout_post, dim3((unsigned)((n_tr * 16 + 255) / 256 + (s->num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_adam_step(const lg_adam_tensor *tensors, int32_t n_tensors, float *lr, float beta1, float beta2, float eps, float max_grad_norm,
                 const float *kl, float desired_kl, float *scratch, void *stream) {
    if (!tensors || !lr || !scratch || n_tensors < 1 || n_tensors > LG_ADAM_MAX_TENSORS) return fail(-1, "bad argument");
    lg::AdamArgs a; memset(&a, 0, sizeof a);
    int64_t max_n = 0;
    for (int k = 0; k < n_tensors; k++) {
        const lg_adam_tensor &t = tensors[k];
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq || !t.step || t.numel <= 0) return fail(-1, "incomplete optimiser tensor");
        a.t[k] = lg::AdamTensor{t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.step, t.numel};
        if (t.numel > max_n) max_n = t.numel;
    }
    a.n_tensors = n_tensors; a.lr = lr; a.kl = kl; a.scratch = scratch;
    a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.max_norm = max_grad_norm; a.desired_kl = desired_kl;
    hipStream_t st = (hipStream_t)stream;
    static_assert(LG_ADAM_SCRATCH_FLOATS >= 2 + LG_ADAM_MAX_TENSORS * LG_ADAM_CHUNKS, "scratch contract");
    const int64_t chunk_len = (max_n + LG_ADAM_CHUNKS - 1) / LG_ADAM_CHUNKS;
    hipLaunchKernelGGL(lg::k_adam_sumsq, dim3(LG_ADAM_CHUNKS, n_tensors), dim3(256), 0, st, a, chunk_len);
    hipLaunchKernelGGL(lg::k_adam_prepare, dim3(1), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(lg::k_adam_update, dim3((unsigned)((max_n + 255) / 256), n_tensors), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int policy_pack_wide(lg_policy *p, const float *const weights[4], const float *const biases[4], hipStream_t st) {
    for (int i = 0; i < 4; i++) {
        const size_t n = (size_t)p->wide_ot[i] * p->wide_ks[i] * 512 + (size_t)p->wide_ot[i] * 32;
        hipLaunchKernelGGL(lg::k_policy_pack_wide, dim3((unsigned)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256)), dim3(256), 0, st, weights[i], biases[i],
                           p->dims[i], p->dims[i + 1], p->wide_ks[i], p->wide_ot[i], i == 0 ? 1 : 0, p->d_wb[i], p->d_bb[i]);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_policy_load_device(lg_policy *p, const float *const weights[4], const float *const biases[4], const float *std, void *stream) {
    if (!p || !weights || !biases || !std) return fail(-1, "null argument");
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < 4; i++) {
        if (!weights[i] || !biases[i]) return fail(-1, "null layer pointer");
        const int in_t = p->tiles[i], out_t = (i < 3) ? p->tiles[i + 1] : 1;
        const size_t n = (size_t)out_t * in_t * 4 * 64 + (size_t)out_t * 4 * 64;
        hipLaunchKernelGGL(k_policy_pack, dim3((unsigned)((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256)), dim3(256), 0, st, weights[i], biases[i],
                           p->dims[i], p->dims[i + 1], in_t, out_t, p->d_w[i], p->d_b[i]);
    }
    if (p->wide) { int rc = policy_pack_wide(p, weights, biases, st); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(p->d_std, std, p->dims[4] * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_policy_create(const int32_t dims[5], const float *const weights[4], const float *const biases[4], const float *std,
                     int device_id, lg_policy **out) {
    if (!dims || !weights || !biases || !std || !out) return fail(-1, "null argument");
    for (int i = 1; i <= 3; i++) if (dims[i] % 16 || dims[i] <= 0 || dims[i] > 512) return fail(-4, "hidden widths must be multiples of 16, <= 512");
    if (dims[0] <= 0 || dims[0] > 256 || dims[4] <= 0 || dims[4] > 16) return fail(-4, "unsupported obs / action width");
    HIP_TRY(hipSetDevice(device_id));
    lg_policy *p = new (std::nothrow) lg_policy();
    if (!p) return fail(-5, "out of host memory");
    memcpy(p->dims, dims, sizeof p->dims); p->device = device_id;
    for (int i = 0; i < 4; i++) { p->d_w[i] = nullptr; p->d_b[i] = nullptr; p->d_wb[i] = nullptr; p->d_bb[i] = nullptr; }
    p->d_std = nullptr;
    p->tiles[0] = (dims[0] + 15) / 16; p->tiles[1] = dims[1] / 16; p->tiles[2] = dims[2] / 16; p->tiles[3] = dims[3] / 16;
    p->wide = dims[1] == 512 && dims[2] == 256 && dims[3] == 128;
    for (int i = 0; i < 4; i++) {
        int in_t = p->tiles[i], out_t = (i < 3) ? p->tiles[i + 1] : 1;
        size_t nw = (size_t)out_t * in_t * 4 * 64, nb = (size_t)out_t * 4 * 64;
        float *hw = (float *)malloc(nw * 4), *hb = (float *)malloc(nb * 4);
        policy_pack_layer(weights[i], biases[i], dims[i], dims[i + 1], in_t, out_t, hw, hb);
        bool ok = hipMalloc(&p->d_w[i], nw * 4) == hipSuccess && hipMalloc(&p->d_b[i], nb * 4) == hipSuccess &&
                  hipMemcpy(p->d_w[i], hw, nw * 4, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p->d_b[i], hb, nb * 4, hipMemcpyHostToDevice) == hipSuccess;
        free(hw); free(hb);
        if (!ok) { lg_policy_destroy(p); return fail(-10, "policy weight upload failed"); }
    }
    if (hipMalloc(&p->d_std, 16 * 4) != hipSuccess || hipMemcpy(p->d_std, std, dims[4] * 4, hipMemcpyHostToDevice) != hipSuccess) {
        lg_policy_destroy(p); return fail(-10, "policy std upload failed");
    }
    if (p->wide) {                                                 // split-bf16 operand stream: raw parameters up, packed on the device
        float *raw_w[4] = {nullptr, nullptr, nullptr, nullptr}, *raw_b[4] = {nullptr, nullptr, nullptr, nullptr};
        bool ok = true;
        for (int i = 0; i < 4 && ok; i++) {
            p->wide_ks[i] = i == 0 ? (dims[0] + 15) / 16 : dims[i] / 16;
            p->wide_ot[i] = (dims[i + 1] + 31) / 32;
            const size_t nw = (size_t)dims[i] * dims[i + 1], nb = (size_t)dims[i + 1];
            ok = hipMalloc(&p->d_wb[i], (size_t)p->wide_ot[i] * p->wide_ks[i] * 1024 * sizeof(__bf16)) == hipSuccess &&
                 hipMalloc(&p->d_bb[i], (size_t)p->wide_ot[i] * 32 * 4) == hipSuccess &&
                 hipMalloc(&raw_w[i], nw * 4) == hipSuccess && hipMalloc(&raw_b[i], nb * 4) == hipSuccess &&
                 hipMemcpy(raw_w[i], weights[i], nw * 4, hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(raw_b[i], biases[i], nb * 4, hipMemcpyHostToDevice) == hipSuccess;
        }
        if (ok) ok = policy_pack_wide(p, raw_w, raw_b, nullptr) == 0 && hipStreamSynchronize(nullptr) == hipSuccess;
        for (int i = 0; i < 4; i++) { if (raw_w[i]) (void)hipFree(raw_w[i]); if (raw_b[i]) (void)hipFree(raw_b[i]); }
        if (!ok) { lg_policy_destroy(p); return fail(-10, "wide policy weight upload failed"); }
    }
    *out = p;
    return 0;
}

void lg_policy_destroy(lg_policy *p) {
    if (!p) return;
    for (int i = 0; i < 4; i++) {
        if (p->d_w[i]) (void)hipFree(p->d_w[i]);
        if (p->d_b[i]) (void)hipFree(p->d_b[i]);
        if (p->d_wb[i]) (void)hipFree(p->d_wb[i]);
        if (p->d_bb[i]) (void)hipFree(p->d_bb[i]);
    }
    if (p->d_std) (void)hipFree(p->d_std);
    delete p;
}

int lg_policy_act(lg_policy *p, const float *obs, float *actions, float *mean, int32_t num_envs, uint64_t seed, int64_t step,
                  const int64_t *step_counter, int32_t deterministic, void *stream) {
    if (!p || !obs || !actions) return fail(-1, "null argument");
    if (num_envs <= 0) return 0;
    PolicyArgs a;
    fill_policy_args(p, a, obs, actions, mean, num_envs, seed, step, step_counter, deterministic);
    dim3 g((num_envs + 15) / 16), b(64 * LG_POLICY_WAVES);
    hipStream_t st = (hipStream_t)stream;
    const int t0 = p->tiles[0], t1 = p->tiles[1], t2 = p->tiles[2], t3 = p->tiles[3];
    if (p->wide && g_wide_precision == 1 && (t0 == 15 || t0 == 11 || t0 == 2 || t0 == 1)) {          // 32 envs per workgroup on the bf16 matrix cores
        lg::PolicyWideArgs w; w.base = a;
        fill_wide_operands(p, w.wb, w.bb);
        if (t0 == 1) { HIP_TRY((hipError_t)lg::launch_policy_act_wide_one_tile(w, st)); return 0; }   // dec game: 16 / 3-512-256-128 (1..16 inputs), lg_dec_game.hip
        dim3 gw((num_envs + LG_PW_ENVS - 1) / LG_PW_ENVS), bw(64 * LG_PW_WAVES);
        if (t0 == 15) hipLaunchKernelGGL((lg::k_policy_act_wide<15, 16, 8, 4>), gw, bw, 0, st, w);     // rough: 235-512-256-128
        else if (t0 == 11) hipLaunchKernelGGL((lg::k_policy_act_wide<11, 16, 8, 4>), gw, bw, 0, st, w);  // cassie: 169-512-256-128
        else hipLaunchKernelGGL((lg::k_policy_act_wide<2, 16, 8, 4>), gw, bw, 0, st, w);               // game: 19-512-256-128 (17..32 inputs)
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (t0 == 3 && t1 == 8 && t2 == 4 && t3 == 2) { HIP_TRY((hipError_t)lg::launch_policy_act_flat(a, st)); return 0; }       // flat: 48-128-64-32, lg_kernels.hip
    else if (t0 == 15 && t1 == 32 && t2 == 16 && t3 == 8) hipLaunchKernelGGL((k_policy_act<15, 32, 16, 8>), g, b, 0, st, a);  // rough: 235-512-256-128
    else if (t0 == 11 && t1 == 32 && t2 == 16 && t3 == 8) hipLaunchKernelGGL((k_policy_act<11, 32, 16, 8>), g, b, 0, st, a);  // cassie: 169-512-256-128
    else if (t0 == 2 && t1 == 32 && t2 == 16 && t3 == 8) hipLaunchKernelGGL((k_policy_act<2, 32, 16, 8>), g, b, 0, st, a);    // game: 19-512-256-128
    else if (t0 == 1 && t1 == 32 && t2 == 16 && t3 == 8) { HIP_TRY((hipError_t)lg::launch_policy_act_one_tile(a, st)); return 0; }   // dec game: 16 / 3-512-256-128, lg_dec_game.hip
    else return fail(-4, "actor widths are not one of the compiled-in shapes (48-128-64-32, 235/169/19/16/3-512-256-128)");
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ GAE scan (PPO rollout post-processing)
__global__ void __launch_bounds__(256) k_gae(const float *__restrict__ rewards, const float *__restrict__ values, const uint8_t *__restrict__ dones,
                                             const float *__restrict__ last_values, float gamma, float lam, float *__restrict__ returns,
                                             float *__restrict__ advantages, int T, int N) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    float adv = 0.0f, nxt = last_values[e];
    for (int t = T - 1; t >= 0; t--) {                 // coalesced across envs at every t
        const size_t i = (size_t)t * N + e;
        const float v = values[i], nd = 1.0f - (float)dones[i];
        const float delta = rewards[i] + nd * gamma * nxt - v;
        adv = delta + nd * gamma * lam * adv;
        returns[i] = adv + v;
        advantages[i] = (adv + v) - v;                 // = returns - values, as the reference computes it
        nxt = v;
    }
}

int lg_gae_returns(const float *rewards, const float *values, const uint8_t *dones, const float *last_values, float gamma, float lam,
                   float *returns, float *advantages, int32_t num_steps, int32_t num_envs, void *stream) {
    if (!rewards || !values || !dones || !last_values || !returns || !advantages) return fail(-1, "null argument");
    if (num_steps <= 0 || num_envs <= 0) return 0;
    hipLaunchKernelGGL(k_gae, dim3((num_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, rewards, values, dones, last_values, gamma, lam,
                       returns, advantages, num_steps, num_envs);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ fused PPO loss + gradient w.r.t. the network outputs
#define LG_PPO_MAX_ACTIONS 16
// 16 lanes per row, one action per lane: the row's actions / old means / old sigmas are 48 contiguous bytes read by one instruction per
// array (one row per lane meant 36 load instructions of 64 scattered lines each: 17.6 us for 24 576 rows), the log-probability and the KL
// are 16-lane butterflies, d_mu leaves coalesced.  A workgroup walks LG_LOSS_ROWS_PER_WG rows (passes unrolled: their gathers overlap) and
// keeps its sums in registers.  Measured 15.9 us at 64 rows per workgroup (32: 17.1, 128: 21.3): what is left is the ~770 same-line
// float atomics (2 wave instructions per workgroup) at ~20 ns each; fewer workgroups trade them for longer serial chains.
#define LG_LOSS_ROWS_PER_WG 64
__global__ void __launch_bounds__(256) k_ppo_loss(const float *__restrict__ mu, const float *__restrict__ stdp, const float *__restrict__ value,
                                                  const int64_t *__restrict__ rows, const float *__restrict__ actions, const float *__restrict__ old_lp,
                                                  const float *__restrict__ old_mu, const float *__restrict__ old_sigma, const float *__restrict__ adv,
                                                  const float *__restrict__ old_values, const float *__restrict__ returns, float clip, float vcoef,
                                                  float ecoef, int clipped_value, float *__restrict__ d_mu, float *__restrict__ d_std,
                                                  float *__restrict__ d_value, float *__restrict__ stats, int mb, int A) {
    __shared__ float red[4 + LG_PPO_MAX_ACTIONS];
    if (threadIdx.x < 4 + LG_PPO_MAX_ACTIONS) red[threadIdx.x] = 0.0f;
    __syncthreads();
    const int a = threadIdx.x & 15, rl = threadIdx.x >> 4;             // action of this lane; row slot 0..15 of the pass
    const float inv_n = 1.0f / (float)mb;
    const bool act_lane = a < A;
    const float sg = act_lane ? stdp[a] : 1.0f, isg = 1.0f / sg, lsg = __logf(sg);
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, gstd = 0.0f;
    const int r_begin = blockIdx.x * LG_LOSS_ROWS_PER_WG, r_end = min(mb, r_begin + LG_LOSS_ROWS_PER_WG);
#pragma unroll 4                                                       // the four passes' gathers in flight together (each pass alone is a ~2.5 us chain)
    for (int i0 = r_begin; i0 < r_end; i0 += 16) {
        const int i = i0 + rl;
        const bool live = i < r_end;
        const int ii = live ? i : r_end - 1;
        const size_t r = (size_t)rows[ii];
        float z = 0.0f, lp = 0.0f, kl = 0.0f;
        if (act_lane) {
            const float m = mu[(size_t)ii * A + a], om = old_mu[r * A + a], os = old_sigma[r * A + a];
            z = (actions[r * A + a] - m) * isg;
            lp = -0.5f * z * z - lsg - 0.918938533f;                                   // log N(a; mu, sigma)
            kl = __logf(sg / os + 1.0e-5f) + (os * os + (om - m) * (om - m)) * (0.5f * isg * isg) - 0.5f;
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { lp += __shfl_xor(lp, o); kl += __shfl_xor(kl, o); }     // every lane of the row holds the sums
        const float ad = adv[r], ratio = __expf(lp - old_lp[r]);
        const float s1 = -ad * ratio, s2 = -ad * fminf(fmaxf(ratio, 1.0f - clip), 1.0f + clip);
        const bool inside = ratio >= 1.0f - clip && ratio <= 1.0f + clip;
        // d max(s1, s2) / d lp: s1 wins (or ties, inside the clamp range) -> -A r; the clamped branch has no gradient outside the range
        const float dlp = (s1 > s2 || inside) ? -ad * ratio : (s1 == s2 ? -0.5f * ad * ratio : 0.0f);
        if (live && act_lane) {
            d_mu[(size_t)i * A + a] = inv_n * dlp * z * isg;                           // d lp / d mu = (a - mu) / sigma^2
            gstd += inv_n * dlp * (z * z - 1.0f) * isg;                                // d lp / d sigma = ((a - mu)^2 / sigma^2 - 1) / sigma
        }
        if (live && a == 0) {
            const float v = value[i], tv = old_values[r], R = returns[r];
            float dv, vl;
            if (clipped_value) {
                const float dvt = v - tv, vc = tv + fminf(fmaxf(dvt, -clip), clip);
                const float v1 = (v - R) * (v - R), v2 = (vc - R) * (vc - R);
                const bool in_v = dvt >= -clip && dvt <= clip;
                vl = fmaxf(v1, v2);
                dv = (v1 > v2 || in_v) ? 2.0f * (v - R) : (v1 == v2 ? (v - R) : 0.0f);
            } else {
                vl = (R - v) * (R - v);
                dv = 2.0f * (v - R);
            }
            d_value[i] = vcoef * inv_n * dv;
            acc0 += fmaxf(s1, s2); acc1 += vl; acc2 += kl;
        }
    }
    // this thread's sums: acc* on the a == 0 lanes (rows rl, rl + 16, ...), gstd for action a.  Fold the 4 row slots of the wave (lanes 16
    // apart), then the waves through LDS, then one atomic per value and workgroup.
#pragma unroll
    for (int o = 32; o >= 16; o >>= 1) { acc0 += __shfl_xor(acc0, o); acc1 += __shfl_xor(acc1, o); acc2 += __shfl_xor(acc2, o); gstd += __shfl_xor(gstd, o); }
    if ((threadIdx.x & 63) < 16) {
        if (a == 0) { atomicAdd(&red[0], acc0); atomicAdd(&red[1], acc1); atomicAdd(&red[2], acc2); }
        if (act_lane) atomicAdd(&red[4 + a], gstd);
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicAdd(stats + threadIdx.x, red[threadIdx.x] * inv_n);
    if (threadIdx.x >= 4 && threadIdx.x < 4 + A) atomicAdd(d_std + (threadIdx.x - 4), red[threadIdx.x]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {                                          // entropy is row-independent: sum_a (0.5 + 0.5 log 2 pi + log sigma_a)
        float H = 0.0f;
        for (int k = 0; k < A; k++) { H += 1.418938533f + __logf(stdp[k]); atomicAdd(d_std + k, -ecoef / stdp[k]); }
        stats[3] = H;
    }
}

__global__ void k_zero2(float *a, int na, float *b, int nb) {
    if ((int)threadIdx.x < na) a[threadIdx.x] = 0.0f;
    if ((int)threadIdx.x < nb) b[threadIdx.x] = 0.0f;
}

int lg_ppo_loss(const float *mu, const float *std, const float *value, const int64_t *rows, const float *actions, const float *old_log_prob,
                const float *old_mu, const float *old_sigma, const float *advantages, const float *old_values, const float *returns, float clip,
                float value_coef, float entropy_coef, int32_t use_clipped_value, float *d_mu, float *d_std, float *d_value, float *stats,
                int32_t mb, int32_t num_actions, void *stream) {
    if (!mu || !std || !value || !rows || !actions || !old_log_prob || !old_mu || !old_sigma || !advantages || !old_values || !returns || !d_mu ||
        !d_std || !d_value || !stats) return fail(-1, "null argument");
    if (num_actions < 1 || num_actions > LG_PPO_MAX_ACTIONS) return fail(-4, "lg_ppo_loss supports 1..16 actions");
    if (mb <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_zero2, dim3(1), dim3(64), 0, st, stats, 4, d_std, (int)num_actions);     // (a kernel, not hipMemsetAsync: replayed inside HIP graphs)
    hipLaunchKernelGGL(k_ppo_loss, dim3((mb + LG_LOSS_ROWS_PER_WG - 1) / LG_LOSS_ROWS_PER_WG), dim3(256), 0, st, mu, std, value, rows, actions, old_log_prob, old_mu, old_sigma, advantages,
                       old_values, returns, clip, value_coef, entropy_coef, (int)use_clipped_value, d_mu, d_std, d_value, stats, (int)mb, (int)num_actions);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
