// lg_memory_host.h -- the host half of a recurrent policy's handles, written once: create / load_device / destroy of a cell memory
// (lg_lstm, lg_lstm_wide, lg_gru), create / load_device / destroy / act of the actor MLP behind one (lg_lstm_actor, lg_lstm_wide_actor),
// and what the step and actor launches share (the sizes of their LDS blocks, the fill of a role and of the actor's arguments).  The
// extern "C" entry points of lg_recurrent.hip, lg_lstm_wide.hip and lg_gru.hip are one-line callers.  Templates and static functions only:
// each library compiles its own copy against its own kernels and error text.  Needs <hip/hip_runtime.h> and lg_recurrent.h.
//
// A cell memory's traits M:
//   Handle                    four int32 (num_in, hidden, ksteps, device) and the two device pointers d_wp, d_bp
//   GATES                     gate rows per unit of w_ih / w_hh / b_ih / b_hh in the torch layout (LSTM 4, GRU 3)
//   MAX_IN, MAX_HIDDEN        the limits of create
//   name(), hidden_note()     the entry-name prefix of the messages ("lg_lstm"), what follows the hidden range in create's message
//   cell_kernel()             the kernel whose dynamic-LDS limit create raises to cell_lds_bytes((MAX_IN + MAX_HIDDEN) / 2)
//   pack(grid, stream, ...)   launches the pack kernel
//   error(code, msg)          stores the message and returns the code (lg::fail in the main library, the library's own refuse elsewhere)
// An actor's traits T: Handle, MAX_HIDDEN, name(), actor_kernel(), pack(grid, stream, ...), act(grid, lds, stream, A), error(code, msg).
#pragma once
#include <stdio.h>

namespace lg {

static size_t cell_lds_bytes(const int ksteps) { return (size_t)2 * ksteps * LG_LSTM_LD * sizeof(float); }
static size_t actor_lds_bytes(const int max_width) { return ((size_t)2 * max_width * LG_LSTM_LD + 32 * 16) * sizeof(float); }

template <class T, class... Args>
static int memory_error(const int code, const char *fmt, Args... args) {
    char msg[512];
    snprintf(msg, sizeof(msg), fmt, args...);
    return T::error(code, msg);
}
#define LG_MEMORY_TRY(T, x) do { hipError_t _e = (x); if (_e != hipSuccess) return lg::memory_error<T>(-10, "HIP error: %s", hipGetErrorString(_e)); } while (0)

// ------------------------------------------------------------------ cell memories
template <class M>
static int memory_pack(typename M::Handle *l, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, hipStream_t stream) {
    const int total = (l->hidden / 32) * l->ksteps * 64 + l->hidden;
    M::pack(dim3((total + 255) / 256), stream, w_ih, w_hh, b_ih, b_hh, (float4 *)l->d_wp, (float4 *)l->d_bp, l->num_in, l->hidden, l->ksteps);
    LG_MEMORY_TRY(M, hipGetLastError());
    return 0;
}

template <class M>
static int memory_create(const int32_t num_in, const int32_t hidden, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                         const int32_t device_id, typename M::Handle **out) {
    if (!out || !w_ih || !w_hh || !b_ih || !b_hh) return memory_error<M>(-1, "%s_create: null argument", M::name());
    *out = nullptr;
    if (num_in < 1 || num_in > M::MAX_IN) return memory_error<M>(-4, "%s_create: num_in must be 1 .. %d", M::name(), M::MAX_IN);
    if (hidden < 32 || hidden > M::MAX_HIDDEN || hidden % 32)
        return memory_error<M>(-4, "%s_create: hidden must be a multiple of 32 in 32 .. %d%s", M::name(), M::MAX_HIDDEN, M::hidden_note());
    LG_MEMORY_TRY(M, hipSetDevice(device_id));
    // the staged [x | h] block of the largest shape is above the 64 KB a kernel gets without asking
    LG_MEMORY_TRY(M, hipFuncSetAttribute(M::cell_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cell_lds_bytes((M::MAX_IN + M::MAX_HIDDEN) / 2)));
    typename M::Handle *l = new typename M::Handle();
    l->num_in = num_in; l->hidden = hidden; l->ksteps = (num_in + hidden + 1) / 2; l->device = device_id;
    l->d_wp = l->d_bp = nullptr;
    const size_t n_ih = (size_t)M::GATES * hidden * num_in, n_hh = (size_t)M::GATES * hidden * hidden, n_b = (size_t)M::GATES * hidden;
    float *raw = nullptr;
    auto body = [&]() -> int {
        LG_MEMORY_TRY(M, hipMalloc(&l->d_wp, (size_t)(hidden / 32) * l->ksteps * 64 * 4 * sizeof(float)));
        LG_MEMORY_TRY(M, hipMalloc(&l->d_bp, (size_t)4 * hidden * sizeof(float)));
        LG_MEMORY_TRY(M, hipMalloc(&raw, (n_ih + n_hh + 2 * n_b) * sizeof(float)));
        LG_MEMORY_TRY(M, hipMemcpy(raw, w_ih, n_ih * sizeof(float), hipMemcpyHostToDevice));
        LG_MEMORY_TRY(M, hipMemcpy(raw + n_ih, w_hh, n_hh * sizeof(float), hipMemcpyHostToDevice));
        LG_MEMORY_TRY(M, hipMemcpy(raw + n_ih + n_hh, b_ih, n_b * sizeof(float), hipMemcpyHostToDevice));
        LG_MEMORY_TRY(M, hipMemcpy(raw + n_ih + n_hh + n_b, b_hh, n_b * sizeof(float), hipMemcpyHostToDevice));
        const int prc = memory_pack<M>(l, raw, raw + n_ih, raw + n_ih + n_hh, raw + n_ih + n_hh + n_b, nullptr);
        if (prc) return prc;
        LG_MEMORY_TRY(M, hipStreamSynchronize(nullptr));
        return 0;
    };
    const int rc = body();
    if (raw) (void)hipFree(raw);
    if (rc) {
        if (l->d_wp) (void)hipFree(l->d_wp);
        if (l->d_bp) (void)hipFree(l->d_bp);
        delete l;
        return rc;
    }
    *out = l;
    return 0;
}

template <class M>
static int memory_load_device(typename M::Handle *l, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, void *stream) {
    if (!l || !w_ih || !w_hh || !b_ih || !b_hh) return memory_error<M>(-1, "%s_load_device: null argument", M::name());
    return memory_pack<M>(l, w_ih, w_hh, b_ih, b_hh, (hipStream_t)stream);
}

template <class M>
static int memory_destroy(typename M::Handle *l) {
    if (!l) return memory_error<M>(-1, "%s_destroy: null handle", M::name());
    (void)hipFree(l->d_wp);
    (void)hipFree(l->d_bp);
    delete l;
    return 0;
}

// an LSTM role of a cell launch from its handle (lg_lstm or lg_lstm_wide) and the caller's buffers
template <class Handle>
static void fill_lstm_role(LstmRole &R, const Handle *l, const float *x, const float *h_in, const float *c_in, float *h_out, float *c_out) {
    R.x = x; R.h_in = h_in; R.c_in = c_in; R.h_out = h_out; R.c_out = c_out;
    R.wp = l->d_wp; R.bp = l->d_bp; R.num_in = l->num_in; R.hidden = l->hidden; R.ksteps = l->ksteps;
}

// what lg_lstm_step and lg_lstm_wide_step refuse before they size a launch, in this order
template <class M>
static int lstm_step_check(const typename M::Handle *l_a, const typename M::Handle *l_c, const float *x_a, const float *x_c,
                           const float *h_in_a, const float *c_in_a, const float *h_out_a, const float *c_out_a,
                           const float *h_in_c, const float *c_in_c, const float *h_out_c, const float *c_out_c, const int32_t num_envs) {
    if (!l_a && !l_c) return memory_error<M>(-1, "%s_step: both handles are null", M::name());
    if (l_a && (!x_a || !h_in_a || !c_in_a || !h_out_a || !c_out_a)) return memory_error<M>(-1, "%s_step: null buffer of the actor memory", M::name());
    if (l_c && (!x_c || !h_in_c || !c_in_c || !h_out_c || !c_out_c)) return memory_error<M>(-1, "%s_step: null buffer of the critic memory", M::name());
    if (num_envs < 1) return memory_error<M>(-2, "%s_step: num_envs must be >= 1", M::name());
    auto aliased = [](const float *h_in, const float *c_in, const float *h_out, const float *c_out) {
        return h_out == h_in || h_out == c_in || c_out == h_in || c_out == c_in || h_out == c_out;
    };
    if ((l_a && aliased(h_in_a, c_in_a, h_out_a, c_out_a)) || (l_c && aliased(h_in_c, c_in_c, h_out_c, c_out_c)))
        return memory_error<M>(-2, "%s_step: h_out / c_out must not alias h_in / c_in (other workgroups read them as the K operand)", M::name());
    if (l_a && l_c && l_a->device != l_c->device) return memory_error<M>(-2, "%s_step: the two memories live on different devices", M::name());
    return 0;
}

// ------------------------------------------------------------------ actor MLPs
template <class T>
static int actor_create(const int32_t dims[5], const int32_t device_id, typename T::Handle **out) {
    if (!dims || !out) return memory_error<T>(-1, "%s_create: null argument", T::name());
    *out = nullptr;
    if (dims[0] < 32 || dims[0] > T::MAX_HIDDEN || dims[0] % 32)
        return memory_error<T>(-4, "%s_create: the input width must be a memory's hidden size (a multiple of 32 in 32 .. %d)", T::name(), T::MAX_HIDDEN);
    for (int i = 1; i <= 3; i++)
        if (dims[i] < 32 || dims[i] > 512 || dims[i] % 32) return memory_error<T>(-4, "%s_create: hidden widths must be multiples of 32 in 32 .. 512", T::name());
    if (dims[4] < 1 || dims[4] > 16) return memory_error<T>(-4, "%s_create: 1 .. 16 actions", T::name());
    LG_MEMORY_TRY(T, hipSetDevice(device_id));
    typename T::Handle *a = new typename T::Handle();
    size_t at = 0;
    a->max_width = 0;
    for (int i = 0; i < 5; i++) {
        a->dims[i] = dims[i]; a->pad[i] = (dims[i] + 31) / 32 * 32;
        if (i < 4 && a->pad[i] > a->max_width) a->max_width = a->pad[i];
    }
    for (int i = 0; i < 4; i++) {
        a->w_off[i] = at; at += (size_t)a->pad[i + 1] * dims[i];
        a->b_off[i] = at; at += (size_t)a->pad[i + 1];
    }
    a->device = device_id; a->d_p = a->d_std = nullptr;
    if (hipFuncSetAttribute(T::actor_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)actor_lds_bytes(512)) != hipSuccess ||
        hipMalloc(&a->d_p, at * sizeof(float)) != hipSuccess || hipMalloc(&a->d_std, 16 * sizeof(float)) != hipSuccess ||
        hipMemset(a->d_p, 0, at * sizeof(float)) != hipSuccess || hipMemset(a->d_std, 0, 16 * sizeof(float)) != hipSuccess) {
        if (a->d_p) (void)hipFree(a->d_p);
        if (a->d_std) (void)hipFree(a->d_std);
        delete a;
        return memory_error<T>(-10, "%s_create: device allocation failed", T::name());
    }
    *out = a;
    return 0;
}

template <class T>
static int actor_load_device(typename T::Handle *a, const float *const weights[4], const float *const biases[4], const float *std, void *stream) {
    if (!a || !weights || !biases || !std) return memory_error<T>(-1, "%s_load_device: null argument", T::name());
    for (int i = 0; i < 4; i++) if (!weights[i] || !biases[i]) return memory_error<T>(-1, "%s_load_device: null layer", T::name());
    for (int i = 0; i < 4; i++) {
        const int total = a->pad[i + 1] * a->dims[i] + a->pad[i + 1];
        T::pack(dim3((total + 255) / 256), (hipStream_t)stream, weights[i], biases[i], a->d_p + a->w_off[i], a->d_p + a->b_off[i], a->dims[i], a->dims[i + 1],
                a->pad[i + 1]);
        LG_MEMORY_TRY(T, hipGetLastError());
    }
    LG_MEMORY_TRY(T, hipMemcpyAsync(a->d_std, std, a->dims[4] * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

template <class T>
static int actor_destroy(typename T::Handle *a) {
    if (!a) return memory_error<T>(-1, "%s_destroy: null handle", T::name());
    (void)hipFree(a->d_p);
    (void)hipFree(a->d_std);
    delete a;
    return 0;
}

// the arguments of an actor chain from its handle (lg_lstm_actor or lg_lstm_wide_actor): the ONE copy, for *_actor_act and for the sampled
// roles of the game tasks' actor launches
template <class Handle>
static void fill_lstm_actor_args(LstmActorArgs &A, const Handle *a, const float *h, float *sample, float *mean, const int num_envs,
                                 const uint64_t seed, const int64_t step, const int64_t *step_counter, const int deterministic) {
    A.h = h; A.p = a->d_p; A.std = a->d_std; A.actions = sample; A.mean = mean; A.step_counter = step_counter;
    A.seed = seed; A.step = step; A.num_envs = num_envs; A.deterministic = deterministic; A.max_width = a->max_width;
    for (int i = 0; i < 5; i++) { A.dims[i] = a->dims[i]; A.pad[i] = a->pad[i]; }
    for (int i = 0; i < 4; i++) { A.w_off[i] = (uint32_t)a->w_off[i]; A.b_off[i] = (uint32_t)a->b_off[i]; }
}

template <class T>
static int actor_act(const typename T::Handle *a, const float *h, float *actions, float *mean, const int32_t num_envs, const uint64_t seed,
                     const int64_t step, const int64_t *step_counter, const int32_t deterministic, void *stream) {
    if (!a || !h || !actions) return memory_error<T>(-1, "%s_act: null argument", T::name());
    if (num_envs < 1) return memory_error<T>(-2, "%s_act: num_envs must be >= 1", T::name());
    LstmActorArgs A = {};
    fill_lstm_actor_args(A, a, h, actions, mean, num_envs, seed, step, step_counter, deterministic);
    T::act(dim3((num_envs + 31) / 32), actor_lds_bytes(a->max_width), (hipStream_t)stream, A);
    LG_MEMORY_TRY(T, hipGetLastError());
    return 0;
}

}  // namespace lg
