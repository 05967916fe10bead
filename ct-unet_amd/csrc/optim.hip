// Everything that walks a list of parameter tensors, for gfx950: fused Adam / AdamW, SGD and RMSprop, the global gradient
// norm and clip coefficient, in-place scaling of a tensor list, the plateau schedule and the loss-scale update.
// One layer underneath all of them: a pointer table passed BY VALUE in the kernel arguments (<= 64 tensors a launch: no
// device-side table to keep in sync, and the launch is graph-capturable), one host walker that cuts a list into tables,
// and one argument check that refuses a bad list before anything is launched.
#include "common.h"

namespace {

constexpr int EW_BLOCK = 256;
constexpr int MAXT = 64;            // tensors per launch (blockIdx.y)

// K pointer slots per tensor, slot-major, and the element counts: 5 slots are 3 KB of kernel arguments.  The slots hold
// what the entry point's ptrs array holds, K per tensor in the same order; each kernel names its own.
template <int K>
struct PtrTable {
    float* q[K][MAXT];
    int64_t n[MAXT];
};

// ------------------------------------------------------------------ the host side of the table
// The one argument check of the table entry points: nothing is launched unless every tensor of the WHOLE list passes.
// need[k]: slot k of a tensor's K pointers must be non-null (a state slot the options do not use may be NULL).
const bool NEED_ALL[5] = {true, true, true, true, true};
int table_check(const char* what, void* const* ptrs, const int64_t* sizes, int n, int K, const bool* need) {
    CTU_REQUIRE(ptrs && sizes && n > 0, "%s: bad argument", what);
    for (int t = 0; t < n; ++t) {
        CTU_REQUIRE(sizes[t] >= 0, "%s: negative size at %d", what, t);
        for (int k = 0; k < K; ++k) {
            void* q = ptrs[(size_t)t * K + k];
            CTU_REQUIRE(q || !need[k], "%s: null tensor pointer at %d (slot %d)", what, t, k);
            CTU_REQUIRE(((uintptr_t)q & 3) == 0, "%s: tensor %d (slot %d) is not 4-byte aligned", what, t, k);
        }
    }
    return CTU_OK;
}

// The launch plan over sizes alone: chunks of MAXT tensors, fn(t0, nt, mx) with mx the chunk's largest size (at least 1);
// stops with fn's first non-zero status.  Workspace sizes and launches both come from this walk.
template <class Fn>
int for_each_chunk(const int64_t* sizes, int n, Fn fn) {
    for (int t0 = 0; t0 < n; t0 += MAXT) {
        const int nt = (n - t0) < MAXT ? (n - t0) : MAXT;
        int64_t mx = 1;
        for (int t = 0; t < nt; ++t)
            if (sizes[t0 + t] > mx) mx = sizes[t0 + t];
        if (int rc = fn(t0, nt, mx)) return rc;
    }
    return CTU_OK;
}

// ... and with each chunk's table filled: fn(tb, nt, mx, t0)
template <int K, class Fn>
int for_each_table(void* const* ptrs, const int64_t* sizes, int n, Fn fn) {
    return for_each_chunk(sizes, n, [&](int t0, int nt, int64_t mx) -> int {
        PtrTable<K> tb;
        for (int t = 0; t < nt; ++t) {
            for (int k = 0; k < K; ++k) tb.q[k][t] = (float*)ptrs[(size_t)(t0 + t) * K + k];
            tb.n[t] = sizes[t0 + t];
        }
        return fn(tb, nt, mx, t0);
    });
}

// grid.x of a table launch: blocks along the chunk's largest tensor, between 1 and cap (the kernels stride over the rest)
inline int table_grid_x(int64_t mx, int64_t elems_per_block, int cap) {
    const int64_t gx = ceil_div64(mx, elems_per_block);
    return gx > cap ? cap : (gx < 1 ? 1 : (int)gx);
}

// ------------------------------------------------------------------ Adam(amsgrad)
// The step counter lives on the device so a replayed graph still advances the bias corrections.
// skip: optional device flag (float[1]); non-zero = this step's gradients overflowed (ctu_scale_tensors found a non-finite
// value while un-scaling fp16 gradients): the whole update is skipped -- parameters, moments AND the step counter stay
// as they are, what torch.amp.GradScaler.step does.  Works inside a replayed graph (the flag is read on the device).
__global__ void adam_step_inc_kernel(float* step, const float* __restrict__ skip) {
    if (skip && skip[0] != 0.f) return;
    step[0] += 1.f;
}

// One body of arithmetic for both entry points.  DEV: the learning rate is a double in device memory, rounded to float
// here exactly where the host call rounds its argument, and the gradient is multiplied by an optional device coefficient
// (gradient clipping) before weight decay, as clip_grad_norm_ scales p.grad before the optimizer reads it.
// slots: param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq
template <bool DEV>
__device__ __forceinline__ void adam_amsgrad_body(const PtrTable<5>& tb, const float* __restrict__ step, float lr, float beta1,
                                                  float beta2, float omb1, float omb2, float eps, float wd, int decoupled,
                                                  const float* __restrict__ skip, const double* __restrict__ dlr,
                                                  const float* __restrict__ gcoef) {
    if (skip && skip[0] != 0.f) return;
    float coef = 1.f;
    bool clip = false;
    if (DEV) {
        lr = (float)dlr[0];
        clip = gcoef != nullptr;
        if (clip) coef = gcoef[0];
    }
    const int t = blockIdx.y;
    const int64_t n = tb.n[t];
    float* __restrict__ p = tb.q[0][t];
    const float* __restrict__ g = tb.q[1][t];
    float* __restrict__ m = tb.q[2][t];
    float* __restrict__ v = tb.q[3][t];
    float* __restrict__ vm = tb.q[4][t];
    // bias corrections in double, like the Python scalars of torch.optim.Adam
    const double st = (double)step[0];
    const float bc1 = (float)(1.0 - pow((double)beta1, st));
    const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, st));
    const float step_size = lr / bc1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float gr = g[i];
        if (DEV && clip) {
            gr *= coef;
            asm volatile("" : "+v"(gr));            // the product is rounded on its own: never contracted into the FMAs below
        }
        float pv = p[i];
        if (wd != 0.f) {
            if (decoupled) pv *= 1.f - lr * wd;     // AdamW
            else gr = fmaf(wd, pv, gr);            // Adam (L2)
        }
        // torch.optim.Adam single-tensor form: lerp for exp_avg, mul/addcmul for exp_avg_sq
        const float mi = m[i] + (gr - m[i]) * omb1;          // omb = 1 - beta formed in double on the host, as torch does
        const float vi = v[i] * beta2 + omb2 * gr * gr;
        const float vmx = fmaxf(vm[i], vi);
        m[i] = mi; v[i] = vi; vm[i] = vmx;
        const float denom = sqrtf(vmx) / bc2_sqrt + eps;
        p[i] = pv - step_size * (mi / denom);
    }
}

__global__ void adam_amsgrad_kernel(PtrTable<5> tb, const float* __restrict__ step, float lr, float beta1, float beta2,
                                    float omb1, float omb2, float eps, float wd, int decoupled, const float* __restrict__ skip) {
    adam_amsgrad_body<false>(tb, step, lr, beta1, beta2, omb1, omb2, eps, wd, decoupled, skip, nullptr, nullptr);
}

__global__ void adam_amsgrad_dev_kernel(PtrTable<5> tb, const float* __restrict__ step, const double* __restrict__ dlr,
                                        float beta1, float beta2, float omb1, float omb2, float eps, float wd, int decoupled,
                                        const float* __restrict__ skip, const float* __restrict__ gcoef) {
    adam_amsgrad_body<true>(tb, step, 0.f, beta1, beta2, omb1, omb2, eps, wd, decoupled, skip, dlr, gcoef);
}

// ------------------------------------------------------------------ SGD and RMSprop
// torch.optim.SGD / torch.optim.RMSprop over a pointer table, launched like the Adam kernels (64 tensors a launch,
// adam_step_inc_kernel in front).  One kernel per rule serves the host and the device learning rate: dlr != NULL
// reads it as (float)dlr[0], rounded where the host call rounds its argument.  A state slot the options do not use is
// NULL and never dereferenced.  Arithmetic is fp32 in the order written; the weight decay is the one fused multiply-add.
struct OptArgs {
    const float* step;                  // device step counter, already incremented for this step (unless it is skipped)
    const double* dlr;                  // NULL: lr below
    const float* gcoef;                 // NULL or the clip coefficient
    const float* skip;                  // NULL or the overflow flag
    float lr, wd, mu;
    float omd;                          // SGD: 1 - dampening;  RMSprop: 1 - alpha (formed in double on the host, as torch does)
    float alpha, eps;                   // RMSprop
    int nesterov, centered, maximize;
};

// what the element rules read besides the tensors, resolved once per thread
struct OptScalars {
    float lr, coef;
    bool clip, first;
};

__device__ __forceinline__ OptScalars opt_scalars(const OptArgs& a) {
    OptScalars s;
    s.lr = a.dlr ? (float)a.dlr[0] : a.lr;
    s.clip = a.gcoef != nullptr;
    s.coef = s.clip ? a.gcoef[0] : 1.f;
    s.first = a.step[0] == 1.f;         // the first APPLIED step: a skipped one left the counter at 0
    return s;
}

__device__ __forceinline__ float opt_grad(float g, float p, const OptArgs& a, const OptScalars& s) {
#pragma clang fp contract(off)
    if (s.clip) g = g * s.coef;
    if (a.maximize) g = -g;
    if (a.wd != 0.f) g = fmaf(a.wd, p, g);         // one rounding, as torch's add(alpha=wd) on the GPU and the Adam kernel:
    return g;                                      // where g cancels to ~0, RMSprop's g / avg follows its last bit
}

__device__ __forceinline__ void sgd_elem(float& p, float g, float& buf, const OptArgs& a, const OptScalars& s) {
#pragma clang fp contract(off)
    g = opt_grad(g, p, a, s);
    if (a.mu != 0.f) {
        buf = s.first ? g : a.mu * buf + a.omd * g;
        g = a.nesterov ? g + a.mu * buf : buf;
    }
    p = p - s.lr * g;
}

__device__ __forceinline__ void rms_elem(float& p, float g, float& sq, float& buf, float& ga, const OptArgs& a,
                                         const OptScalars& s) {
#pragma clang fp contract(off)
    g = opt_grad(g, p, a, s);
    sq = a.alpha * sq + a.omd * g * g;
    float avg;
    if (a.centered) {
        ga = ga + a.omd * (g - ga);
        avg = sqrtf(sq - ga * ga) + a.eps;
    } else {
        avg = sqrtf(sq) + a.eps;
    }
    if (a.mu > 0.f) {
        buf = a.mu * buf + g / avg;
        p = p - s.lr * buf;
    } else {
        p = p - s.lr * (g / avg);
    }
}

// How one tensor's n elements split into a scalar head, 16-byte groups and a scalar tail.  Pointers are only 4-byte aligned
// (a parameter may be a view at an odd float offset of its storage): the vector body exists when every pointer in use sits
// at the same offset within 16 bytes, so that one head aligns them all; otherwise the whole tensor goes the scalar way.
struct OptSpan {
    int64_t head, n4;
};

__device__ __forceinline__ OptSpan opt_span(int64_t n, const void* p, const void* g, const void* s0, const void* s1,
                                            const void* s2) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p) & 15;
    bool same = (reinterpret_cast<uintptr_t>(g) & 15) == a;
    if (s0) same = same && (reinterpret_cast<uintptr_t>(s0) & 15) == a;
    if (s1) same = same && (reinterpret_cast<uintptr_t>(s1) & 15) == a;
    if (s2) same = same && (reinterpret_cast<uintptr_t>(s2) & 15) == a;
    OptSpan sp;
    if (!same) { sp.head = n; sp.n4 = 0; return sp; }
    const int64_t h = (int64_t)(((16 - a) & 15) >> 2);
    sp.head = h < n ? h : n;
    sp.n4 = (n - sp.head) >> 2;
    return sp;
}

// slots: param, grad, momentum_buffer
__global__ __launch_bounds__(EW_BLOCK) void sgd_kernel(PtrTable<3> tb, OptArgs a) {
    if (a.skip && a.skip[0] != 0.f) return;
    const OptScalars s = opt_scalars(a);
    const int t = blockIdx.y;
    const int64_t n = tb.n[t];
    float* __restrict__ p = tb.q[0][t];
    const float* __restrict__ g = tb.q[1][t];
    float* __restrict__ b = a.mu != 0.f ? tb.q[2][t] : nullptr;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    const OptSpan sp = opt_span(n, p, g, b, nullptr, nullptr);
    auto scalar = [&](int64_t i) {
        float pv = p[i], bv = b ? b[i] : 0.f;
        sgd_elem(pv, g[i], bv, a, s);
        if (b) b[i] = bv;
        p[i] = pv;
    };
    for (int64_t i = tid; i < sp.head; i += nthr) scalar(i);
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p + sp.head);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + sp.head);
    float4* __restrict__ b4 = b ? reinterpret_cast<float4*>(b + sp.head) : nullptr;
    for (int64_t q = tid; q < sp.n4; q += nthr) {
        float4 pv = p4[q], bv = b4 ? b4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 gv = g4[q];
        sgd_elem(pv.x, gv.x, bv.x, a, s); sgd_elem(pv.y, gv.y, bv.y, a, s);
        sgd_elem(pv.z, gv.z, bv.z, a, s); sgd_elem(pv.w, gv.w, bv.w, a, s);
        if (b4) b4[q] = bv;
        p4[q] = pv;
    }
    for (int64_t i = sp.head + (sp.n4 << 2) + tid; i < n; i += nthr) scalar(i);
}

// slots: param, grad, square_avg, momentum_buffer, grad_avg
__global__ __launch_bounds__(EW_BLOCK) void rmsprop_kernel(PtrTable<5> tb, OptArgs a) {
    if (a.skip && a.skip[0] != 0.f) return;
    const OptScalars s = opt_scalars(a);
    const int t = blockIdx.y;
    const int64_t n = tb.n[t];
    float* __restrict__ p = tb.q[0][t];
    const float* __restrict__ g = tb.q[1][t];
    float* __restrict__ sq = tb.q[2][t];
    float* __restrict__ b = a.mu > 0.f ? tb.q[3][t] : nullptr;
    float* __restrict__ ga = a.centered ? tb.q[4][t] : nullptr;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    const OptSpan sp = opt_span(n, p, g, sq, b, ga);
    auto scalar = [&](int64_t i) {
        float pv = p[i], sv = sq[i], bv = b ? b[i] : 0.f, av = ga ? ga[i] : 0.f;
        rms_elem(pv, g[i], sv, bv, av, a, s);
        sq[i] = sv;
        if (b) b[i] = bv;
        if (ga) ga[i] = av;
        p[i] = pv;
    };
    for (int64_t i = tid; i < sp.head; i += nthr) scalar(i);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p + sp.head);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + sp.head);
    float4* __restrict__ s4 = reinterpret_cast<float4*>(sq + sp.head);
    float4* __restrict__ b4 = b ? reinterpret_cast<float4*>(b + sp.head) : nullptr;
    float4* __restrict__ a4 = ga ? reinterpret_cast<float4*>(ga + sp.head) : nullptr;
    for (int64_t q = tid; q < sp.n4; q += nthr) {
        float4 pv = p4[q], sv = s4[q], bv = b4 ? b4[q] : z4, av = a4 ? a4[q] : z4;
        const float4 gv = g4[q];
        rms_elem(pv.x, gv.x, sv.x, bv.x, av.x, a, s); rms_elem(pv.y, gv.y, sv.y, bv.y, av.y, a, s);
        rms_elem(pv.z, gv.z, sv.z, bv.z, av.z, a, s); rms_elem(pv.w, gv.w, sv.w, bv.w, av.w, a, s);
        s4[q] = sv;
        if (b4) b4[q] = bv;
        if (a4) a4[q] = av;
        p4[q] = pv;
    }
    for (int64_t i = sp.head + (sp.n4 << 2) + tid; i < n; i += nthr) scalar(i);
}

// ------------------------------------------------------------------ global gradient norm and clip coefficient
// torch.nn.utils.clip_grad_norm_ (norm_type 2, error_if_nonfinite=False) over a pointer table, in two launches and in a
// fixed order: per-thread double sums of g*g, a fixed-order tree per block, one float partial per block (stage one);
// one block sums the partials in double and writes the norm and the coefficient (stage two).
inline int grad_norm_gx(int64_t mx) { return table_grid_x(mx, EW_BLOCK * 16, 64); }      // four 16-byte loads per thread and trip

__device__ __forceinline__ double block_sum_fixed(double s, double* r) {
    r[threadIdx.x] = s;
    __syncthreads();
    for (int o = EW_BLOCK / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) r[threadIdx.x] += r[threadIdx.x + o];
        __syncthreads();
    }
    return r[0];
}

// slot: grad
__global__ void grad_sqsum_kernel(PtrTable<1> tb, float* __restrict__ partials) {
    __shared__ double r[EW_BLOCK];
    const int t = blockIdx.y;
    const float* __restrict__ g = tb.q[0][t];
    const int64_t n = tb.n[t];
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    double s = 0.0;
    // 16-byte loads when the base allows it (a view at an odd offset of its storage is only 4-byte aligned), scalar tail
    const int64_t n4 = ((reinterpret_cast<uintptr_t>(g) & 15) == 0) ? (n >> 2) : 0;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    for (int64_t i = tid; i < n4; i += nthr) {
        const float4 q = g4[i];
        s += (double)q.x * (double)q.x; s += (double)q.y * (double)q.y;
        s += (double)q.z * (double)q.z; s += (double)q.w * (double)q.w;
    }
    for (int64_t i = (n4 << 2) + tid; i < n; i += nthr) s += (double)g[i] * (double)g[i];
    const double tot = block_sum_fixed(s, r);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (float)tot;
}

__global__ void grad_clip_coef_kernel(const float* __restrict__ partials, int nb, float max_norm, float* __restrict__ norm_out,
                                      float* __restrict__ coef_out) {
    __shared__ double r[EW_BLOCK];
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += blockDim.x) s += (double)partials[b];
    const double tot = block_sum_fixed(s, r);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(tot);
        const float c = max_norm / (norm + 1e-6f);
        norm_out[0] = norm;
        coef_out[0] = c > 1.f ? 1.f : c;            // torch.clamp(max=1): a NaN norm stays a NaN coefficient
    }
}

// ------------------------------------------------------------------ ReduceLROnPlateau on the device
// torch.optim.lr_scheduler.ReduceLROnPlateau.step(float(metric)) for one parameter group on one thread, in double, with
// torch's own expressions (_is_better, _reduce_lr), so the learning rate follows torch's to the last bit.
// state[0] = best; counters = {num_bad_epochs, cooldown_counter, last_epoch, number of reductions}.
__global__ void plateau_update_kernel(const float* __restrict__ metric, double* lr, double* state, int32_t* counters,
                                      int mode_max, int threshold_rel, double factor, int patience, double threshold,
                                      int cooldown, double min_lr, double eps) {
#pragma clang fp contract(off)
    const double cur = (double)metric[0];
    const double best = state[0];
    int bad = counters[0], cool = counters[1];
    counters[2] += 1;
    bool better;
    if (!mode_max && threshold_rel) better = cur < best * (1.0 - threshold);
    else if (!mode_max) better = cur < best - threshold;
    else if (threshold_rel) better = cur > best * (threshold + 1.0);
    else better = cur > best + threshold;              // (a NaN metric compares false: never better)
    if (better) { state[0] = cur; bad = 0; }
    else bad += 1;
    if (cool > 0) { cool -= 1; bad = 0; }               // bad epochs do not count during cooldown
    if (bad > patience) {
        const double old_lr = lr[0];
        const double scaled = old_lr * factor;
        const double new_lr = scaled > min_lr ? scaled : min_lr;          // Python's max(scaled, min_lr)
        if (old_lr - new_lr > eps) { lr[0] = new_lr; counters[3] += 1; }
        cool = cooldown;
        bad = 0;
    }
    counters[0] = bad;
    counters[1] = cool;
}

// ------------------------------------------------------------------ scaling a tensor list in place
// nonfinite: optional device flag (float[1]) set to 1 when any scaled value is inf / NaN (the fp16 backward overflowed)
// DEV: the factor is the reciprocal of the device loss scale *dscale (dynamic loss scaling), formed the way
// torch.amp.GradScaler forms it (scale.double().reciprocal().float()): one uniform scalar load per block
// slot: the tensor
template <bool DEV>
__global__ void scale_tensors_kernel(PtrTable<1> tb, float s, const float* __restrict__ dscale, float* __restrict__ nonfinite) {
    if (DEV) s = (float)(1.0 / (double)dscale[0]);
    const int t = blockIdx.y;
    float* __restrict__ p = tb.q[0][t];
    const int64_t n = tb.n[t];
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = p[i] * s;
        p[i] = v;
        bad |= !(fabsf(v) <= 3.4028234e38f);            // inf or NaN
    }
    if (nonfinite && bad) nonfinite[0] = 1.f;          // (every writer stores the same value)
}

// ------------------------------------------------------------------ dynamic loss scale
// torch._amp_update_scale_ on one thread: back off (and restart the growth count) after an overflowed step, grow after
// `interval` clean steps in a row unless the grown scale would not be finite in float32.  Then count the skipped step and
// clear found_inf: in dynamic mode this is the only place the flag is cleared, so every backward pass of a step (gradient
// accumulation) and the ranks' combined flag of a distributed step reach this decision.
__global__ void loss_scale_update_kernel(float* scale, int32_t* growth_tracker, float* found_inf, float* skipped,
                                         float growth, float backoff, int interval) {
    const float s = scale[0];
    const bool inf = found_inf[0] != 0.f;
    if (inf) {
        scale[0] = (float)((double)s * (double)backoff);
        growth_tracker[0] = 0;
        skipped[0] += 1.f;
    } else {
        const int successful = growth_tracker[0] + 1;
        if (successful == interval) {
            const float grown = (float)((double)s * (double)growth);
            if (isfinite(grown)) scale[0] = grown;
            growth_tracker[0] = 0;
        } else {
            growth_tracker[0] = successful;
        }
    }
    found_inf[0] = 0.f;
}

// =================================================================== host launchers
// What the three optimizers share in front of their table launches: the checks, then the step counter.
int opt_begin(const char* what, void* const* ptrs, const int64_t* sizes, int n, float* step, int K, const bool* need,
              const float* skip_flag, hipStream_t st) {
    CTU_REQUIRE(step, "%s: bad argument", what);
    if (int rc = table_check(what, ptrs, sizes, n, K, need)) return rc;
    adam_step_inc_kernel<<<1, 1, 0, st>>>(step, skip_flag);
    CTU_CHECK_LAUNCH("adam_step_inc");
    return CTU_OK;
}

inline int opt_grid_x(int64_t mx) { return table_grid_x(mx, EW_BLOCK * 4, 128); }

// both Adam entry points: dlr != NULL launches the device-learning-rate kernel
int adam_launch(const char* what, void* const* ptrs, const int64_t* sizes, int n, float* step, const double* dlr, double lr,
                double beta1, double beta2, double eps, double weight_decay, int decoupled, const float* grad_coef,
                const float* skip_flag, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int rc = opt_begin(what, ptrs, sizes, n, step, 5, NEED_ALL, skip_flag, st)) return rc;
    const float b1 = (float)beta1, b2 = (float)beta2, omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
    return for_each_table<5>(ptrs, sizes, n, [&](const PtrTable<5>& tb, int nt, int64_t mx, int) -> int {
        const dim3 grid(opt_grid_x(mx), nt);
        if (dlr)
            adam_amsgrad_dev_kernel<<<grid, EW_BLOCK, 0, st>>>(tb, step, dlr, b1, b2, omb1, omb2, (float)eps,
                                                               (float)weight_decay, decoupled, skip_flag, grad_coef);
        else
            adam_amsgrad_kernel<<<grid, EW_BLOCK, 0, st>>>(tb, step, (float)lr, b1, b2, omb1, omb2, (float)eps,
                                                           (float)weight_decay, decoupled, skip_flag);
        CTU_CHECK_LAUNCH(what);
        return CTU_OK;
    });
}

template <bool DEV>
int scale_tensors_impl(const char* what, void* const* ptrs, const int64_t* sizes, int n, float sc, const float* dscale,
                       float* nonfinite_flag, void* stream) {
    if (int rc = table_check(what, ptrs, sizes, n, 1, NEED_ALL)) return rc;
    return for_each_table<1>(ptrs, sizes, n, [&](const PtrTable<1>& tb, int nt, int64_t mx, int) -> int {
        const int gx = table_grid_x(mx, EW_BLOCK * 4, 2048);        // (dx of a 256^3 two-channel input is 134 MB)
        scale_tensors_kernel<DEV><<<dim3(gx, nt), EW_BLOCK, 0, (hipStream_t)stream>>>(tb, sc, dscale, nonfinite_flag);
        CTU_CHECK_LAUNCH("scale_tensors");
        return CTU_OK;
    });
}

}  // namespace

// =================================================================== C ABI
extern "C" int ctu_adam_amsgrad(void* const* ptrs, const int64_t* sizes, int n, float* step, double lr, double beta1,
                                double beta2, double eps, double weight_decay, int decoupled, const float* skip_flag, void* stream) {
    return adam_launch("adam_amsgrad", ptrs, sizes, n, step, nullptr, lr, beta1, beta2, eps, weight_decay, decoupled, nullptr,
                       skip_flag, stream);
}

extern "C" int ctu_adam_amsgrad_dev(void* const* ptrs, const int64_t* sizes, int n, float* step, const double* lr, double beta1,
                                    double beta2, double eps, double weight_decay, int decoupled, const float* grad_coef,
                                    const float* skip_flag, void* stream) {
    CTU_REQUIRE(lr, "adam_amsgrad_dev: bad argument");
    return adam_launch("adam_amsgrad_dev", ptrs, sizes, n, step, lr, 0.0, beta1, beta2, eps, weight_decay, decoupled, grad_coef,
                       skip_flag, stream);
}

extern "C" int ctu_sgd(void* const* ptrs, const int64_t* sizes, int n, float* step, const double* lr_dev, double lr,
                       double momentum, double dampening, double weight_decay, int nesterov, int maximize,
                       const float* grad_coef, const float* skip_flag, void* stream) {
    CTU_REQUIRE(!nesterov || (momentum != 0.0 && dampening == 0.0),
                "sgd: Nesterov momentum requires a momentum and zero dampening (momentum=%g dampening=%g)", momentum, dampening);
    const bool need[3] = {true, true, momentum != 0.0};
    hipStream_t st = (hipStream_t)stream;
    if (int rc = opt_begin("sgd", ptrs, sizes, n, step, 3, need, skip_flag, st)) return rc;
    OptArgs a = {};
    a.step = step; a.dlr = lr_dev; a.gcoef = grad_coef; a.skip = skip_flag;
    a.lr = (float)lr; a.wd = (float)weight_decay; a.mu = (float)momentum; a.omd = (float)(1.0 - dampening);
    a.nesterov = nesterov != 0; a.maximize = maximize != 0;
    return for_each_table<3>(ptrs, sizes, n, [&](const PtrTable<3>& tb, int nt, int64_t mx, int) -> int {
        sgd_kernel<<<dim3(opt_grid_x(mx), nt), EW_BLOCK, 0, st>>>(tb, a);
        CTU_CHECK_LAUNCH("sgd");
        return CTU_OK;
    });
}

extern "C" int ctu_rmsprop(void* const* ptrs, const int64_t* sizes, int n, float* step, const double* lr_dev, double lr,
                           double alpha, double eps, double weight_decay, double momentum, int centered, int maximize,
                           const float* grad_coef, const float* skip_flag, void* stream) {
    const bool need[5] = {true, true, true, momentum != 0.0, centered != 0};
    hipStream_t st = (hipStream_t)stream;
    if (int rc = opt_begin("rmsprop", ptrs, sizes, n, step, 5, need, skip_flag, st)) return rc;
    OptArgs a = {};
    a.step = step; a.dlr = lr_dev; a.gcoef = grad_coef; a.skip = skip_flag;
    a.lr = (float)lr; a.wd = (float)weight_decay; a.mu = (float)momentum; a.omd = (float)(1.0 - alpha);
    a.alpha = (float)alpha; a.eps = (float)eps;
    a.centered = centered != 0; a.maximize = maximize != 0;
    return for_each_table<5>(ptrs, sizes, n, [&](const PtrTable<5>& tb, int nt, int64_t mx, int) -> int {
        rmsprop_kernel<<<dim3(opt_grid_x(mx), nt), EW_BLOCK, 0, st>>>(tb, a);
        CTU_CHECK_LAUNCH("rmsprop");
        return CTU_OK;
    });
}

extern "C" int ctu_grad_norm_num_blocks(const int64_t* sizes, int n) {
    if (!sizes || n <= 0 || n > (1 << 20)) return 0;           // (64 blocks per tensor at most: the count fits an int)
    int nb = 0;
    for_each_chunk(sizes, n, [&](int, int nt, int64_t mx) -> int { nb += grad_norm_gx(mx) * nt; return CTU_OK; });
    return nb;
}

extern "C" int ctu_grad_clip_coef(void* const* gptrs, const int64_t* sizes, int n, float max_norm, float* partials_ws,
                                  float* norm_out, float* coef_out, void* stream) {
    CTU_REQUIRE(n <= (1 << 20) && partials_ws && norm_out && coef_out, "grad_clip_coef: bad argument");
    if (int rc = table_check("grad_clip_coef", gptrs, sizes, n, 1, NEED_ALL)) return rc;
    hipStream_t st = (hipStream_t)stream;
    int64_t nb = 0;
    const int rc = for_each_table<1>(gptrs, sizes, n, [&](const PtrTable<1>& tb, int nt, int64_t mx, int) -> int {
        const int gx = grad_norm_gx(mx);
        grad_sqsum_kernel<<<dim3(gx, nt), EW_BLOCK, 0, st>>>(tb, partials_ws + nb);
        CTU_CHECK_LAUNCH("grad_sqsum");
        nb += (int64_t)gx * nt;
        return CTU_OK;
    });
    if (rc) return rc;
    grad_clip_coef_kernel<<<1, EW_BLOCK, 0, st>>>(partials_ws, (int)nb, max_norm, norm_out, coef_out);
    CTU_CHECK_LAUNCH("grad_clip_coef");
    return CTU_OK;
}

extern "C" int ctu_plateau_update(const float* metric, double* lr, double* state, int32_t* counters, int mode_max,
                                  int threshold_rel, double factor, int patience, double threshold, int cooldown, double min_lr,
                                  double eps, void* stream) {
    CTU_REQUIRE(metric && lr && state && counters, "plateau_update: null pointer");
    CTU_REQUIRE(factor < 1.0 && patience >= 0 && cooldown >= 0, "plateau_update: factor=%g patience=%d cooldown=%d", factor,
                patience, cooldown);
    plateau_update_kernel<<<1, 1, 0, (hipStream_t)stream>>>(metric, lr, state, counters, mode_max, threshold_rel, factor,
                                                           patience, threshold, cooldown, min_lr, eps);
    CTU_CHECK_LAUNCH("plateau_update");
    return CTU_OK;
}

extern "C" int ctu_scale_tensors(void* const* ptrs, const int64_t* sizes, int n, float sc, float* nonfinite_flag, void* stream) {
    return scale_tensors_impl<false>("scale_tensors", ptrs, sizes, n, sc, nullptr, nonfinite_flag, stream);
}

extern "C" int ctu_unscale_tensors(void* const* ptrs, const int64_t* sizes, int n, const float* scale, float* found_inf,
                                   void* stream) {
    CTU_REQUIRE(scale && found_inf, "unscale_tensors: bad argument");
    return scale_tensors_impl<true>("unscale_tensors", ptrs, sizes, n, 1.f, scale, found_inf, stream);
}

extern "C" int ctu_loss_scale_update(float* scale, int32_t* growth_tracker, float* found_inf, float* skipped, float growth,
                                     float backoff, int interval, void* stream) {
    CTU_REQUIRE(scale && growth_tracker && found_inf && skipped, "loss_scale_update: null pointer");
    CTU_REQUIRE(growth > 1.f && backoff > 0.f && backoff < 1.f && interval >= 1,
                "loss_scale_update: growth=%g backoff=%g interval=%d", (double)growth, (double)backoff, interval);
    loss_scale_update_kernel<<<1, 1, 0, (hipStream_t)stream>>>(scale, growth_tracker, found_inf, skipped, growth, backoff, interval);
    CTU_CHECK_LAUNCH("loss_scale_update");
    return CTU_OK;
}
