// rg_returns.hip -- returns and advantages of a [T, N] rollout on the device (rg_gae, rg_vtrace; gfx950): ONE launch for the whole rollout.
//
//   k_gae<F>    : one env per lane, consecutive envs on consecutive lanes (every row access is coalesced); the lane keeps adv_next and v_next in registers and
//                 walks t from T - 1 down to 0
//   k_vtrace<F> : the same shape with the two log-probability rows and three words of state
//
// F says which optional arrays are present (RET_VALUE | RET_DONE | RET_TRUNC | RET_TV) and O which outputs (1, 2 or both), so no load and no store stands
// behind a runtime test (a test inside the rounds makes the compiler's count of the loads in flight a guess, and its waits drain the pipeline): the recurrence is a short
// dependent chain, the loads do not depend on it, and the kernel is worth what its loads in flight are worth.  A software pipeline in registers, no LDS: the
// rows of the next DEPTH steps are requested before the oldest is consumed (DEPTH = RG_RET_DEPTH for rows of at most four words, half of it above; a
// compile-time ring, every slot index a constant).  Nothing is read or written past column N - 1 or outside rows 0 .. T - 1: a lane past N - 1 leaves at
// once, and every load and store of row t stands behind t >= 0.  Index arithmetic is 64-bit.
//
// An output may be exactly one of the [T, N] float inputs: the lane has read element (t, n) before it writes it, and reads no other lane's element.  So no
// pointer here is __restrict__.
//
// RG_RET_ENVS (1, 2 or 4; the product: 1) is a measurement knob (tools/bench_returns.py): a lane takes that many adjacent envs with one wider load per array,
// where N is a multiple of it and every array is aligned to it; the launcher falls back to one env per lane anywhere else.
//
// A library of its own (librogue_gym_returns.so, which librogue_gym_hip.so links).  The rule is rg_returns.h's, shared with the host twins (rg_gae_host,
// rg_vtrace_host); kernel and twin agree bit for bit.
#include "rg_device.h"
#include "rg_returns.h"

#ifndef RG_RET_DEPTH
#define RG_RET_DEPTH 16
#endif
#ifndef RG_RET_ENVS
#define RG_RET_ENVS 1
#endif

enum { RET_VALUE = 1, RET_DONE = 2, RET_TRUNC = 4, RET_TV = 8 };

struct RetIo {
    const float *reward, *value, *last_value, *tv, *lb, *lt;
    const uint8_t *done, *trunc;
    float *out_a, *out_b;   // (adv, ret) or (vs, pg_adv), each nullable
};

// E adjacent floats / bytes of a row as one load
template <int E> struct RetVec { typedef float F; typedef uint8_t B; };
template <> struct RetVec<2> { typedef float F __attribute__((ext_vector_type(2))); typedef uint16_t B; };
template <> struct RetVec<4> { typedef float F __attribute__((ext_vector_type(4))); typedef uint32_t B; };
template <int E> __device__ __forceinline__ float ret_get(const typename RetVec<E>::F &v, int i) {
    if constexpr (E == 1) return v;
    else return v[i];
}
template <int E> __device__ __forceinline__ void ret_set(typename RetVec<E>::F &v, int i, float f) {
    if constexpr (E == 1) v = f;
    else v[i] = f;
}

// v_next in a register of its own.  The rule's v_next = v would keep the slot's register alive into the next step, the slot's next row would land in another
// register, and the compiler would turn the whole ring once per round, behind a wait for every value load in flight.
__device__ __forceinline__ float ret_own(float v) {
    float c;
    asm volatile("v_mov_b32 %0, %1" : "=&v"(c) : "v"(v));
    return c;
}

// what a lane holds of one row: only the members its F names are ever loaded or looked at
template <int E> struct RetSlot { typename RetVec<E>::F r, v, tv, lb, lt; typename RetVec<E>::B d, tr; };

template <int F, bool VT, int E>
__device__ __forceinline__ void ret_load(RetSlot<E> &s, const RetIo &io, int64_t at, uint32_t lo) {
    typedef typename RetVec<E>::F FV;
    typedef typename RetVec<E>::B BV;
    s.r = *reinterpret_cast<const FV *>(io.reward + at + lo);
    if constexpr ((F & RET_VALUE) != 0) s.v = *reinterpret_cast<const FV *>(io.value + at + lo);
    if constexpr ((F & RET_DONE) != 0) s.d = *reinterpret_cast<const BV *>(io.done + at + lo);
    if constexpr ((F & RET_TRUNC) != 0) s.tr = *reinterpret_cast<const BV *>(io.trunc + at + lo);
    if constexpr ((F & RET_TV) != 0) s.tv = *reinterpret_cast<const FV *>(io.tv + at + lo);
    if constexpr (VT) {
        s.lb = *reinterpret_cast<const FV *>(io.lb + at + lo);
        s.lt = *reinterpret_cast<const FV *>(io.lt + at + lo);
    }
}
template <int F, int E>
__device__ __forceinline__ RgRetRow ret_row(const RetSlot<E> &s, int i) {
    RgRetRow x = {ret_get<E>(s.r, i), 0.0f, 0.0f, false, false, (F & RET_TV) != 0};
    if constexpr ((F & RET_VALUE) != 0) x.v = ret_get<E>(s.v, i);
    if constexpr ((F & RET_DONE) != 0) x.d = ((s.d >> (8 * i)) & 0xffu) != 0;
    if constexpr ((F & RET_TRUNC) != 0) x.tr = ((s.tr >> (8 * i)) & 0xffu) != 0;
    if constexpr ((F & RET_TV) != 0) x.tv = ret_get<E>(s.tv, i);
    return x;
}

template <int F, bool VT> constexpr int ret_words() {
    return 1 + ((F & RET_VALUE) ? 1 : 0) + ((F & RET_DONE) ? 1 : 0) + ((F & RET_TRUNC) ? 1 : 0) + ((F & RET_TV) ? 1 : 0) + (VT ? 2 : 0);
}
template <int F, bool VT> constexpr int ret_depth() { return ret_words<F, VT>() <= 4 ? RG_RET_DEPTH : (RG_RET_DEPTH / 2 < 2 ? 2 : RG_RET_DEPTH / 2); }

// The scan of E adjacent columns from column `lo` of the block's stretch: every pointer of io already stands at the block's first column, so a row's address is
// a wave-uniform base (scalar registers) plus the lane's 32-bit offset, and a load in flight holds no address registers of its own.  Three stretches: the first DEPTH rows are requested; while every row of the next round exists the ring turns
// with unconditional loads; the last rounds (fewer than 2 * DEPTH rows) test each row.
template <int F, bool VT, int O, int E>
__device__ __forceinline__ void ret_scan(const RetIo &io, int64_t T, int64_t N, uint32_t lo, float gamma, float lam_or_gl, const RgVtBars &bars) {
    typedef typename RetVec<E>::F FV;
    constexpr int D = ret_depth<F, VT>();
    RgGaeState g[E];
    RgVtState w[E];
#pragma unroll
    for (int i = 0; i < E; i++) {
        const float lv = io.last_value ? io.last_value[lo + i] : 0.0f;
        g[i] = {0.0f, lv};
        w[i] = {0.0f, lv, lv};
    }
    RetSlot<E> ring[D] = {};   // (members that F does not name are never loaded: they fold away)
    int64_t t = T - 1;   // the row slot 0 holds
    // Rows are requested and consumed in one order, T - 1 down to 0, so two running element offsets serve every address: `ld` of the next row to request, `st`
    // of the next row to consume.  Each is made opaque after its step: otherwise the unrolled rounds get an induction pointer per load, and those spill.
    int64_t ld = t * N, st = t * N;
    auto request = [&](RetSlot<E> &slot) {
        ret_load<F, VT, E>(slot, io, ld, lo);
        ld -= N;
        asm volatile("" : "+s"(ld));
    };
    auto consume = [&](const RetSlot<E> &cur) {
        FV a, b;
#pragma unroll
        for (int i = 0; i < E; i++) {
            const RgRetRow x = ret_row<F, E>(cur, i);
            RgRetPair o;
            if constexpr (VT) {
                o = rg_vtrace_step(w[i], x, ret_get<E>(cur.lb, i), ret_get<E>(cur.lt, i), gamma, lam_or_gl, bars);
                w[i].v_next = ret_own(w[i].v_next);
            } else {
                o = rg_gae_step(g[i], x, gamma, lam_or_gl);
                g[i].v_next = ret_own(g[i].v_next);
            }
            ret_set<E>(a, i, o.a);
            ret_set<E>(b, i, o.b);
        }
        if constexpr ((O & 1) != 0) *reinterpret_cast<FV *>(io.out_a + st + lo) = a;
        if constexpr ((O & 2) != 0) *reinterpret_cast<FV *>(io.out_b + st + lo) = b;
        st -= N;
        asm volatile("" : "+s"(st));
    };
    if (t >= 2 * D - 1) {   // (no test stands between these requests and the rounds below: the compiler counts the loads in flight exactly)
#pragma unroll
        for (int j = 0; j < D; j++) request(ring[j]);
        for (; t >= 2 * D - 1; t -= D) {
#pragma unroll
            for (int j = 0; j < D; j++) {
                consume(ring[j]);   // (first: the slot's register is free when its next row is requested, and the ring stays where it is)
                request(ring[j]);
                // Steps stay in order.  Left alone, the scheduler lifts the loads' part of every step of the round (delta needs no state) to the top of the
                // round, behind a wait for ALL loads in flight: the pipeline would drain once per round.
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < D; j++)
            if (t - j >= 0) request(ring[j]);
    }
    for (; t >= 0; t -= D) {
#pragma unroll
        for (int j = 0; j < D; j++) {
            if (t - j < 0) break;
            const RetSlot<E> cur = ring[j];
            if (t - j - D >= 0) request(ring[j]);
            consume(cur);
        }
    }
}

// the block's io: every array moved to the block's first column nb (NULL stays NULL)
__device__ __forceinline__ RetIo ret_block_io(const RetIo &io, int64_t nb) {
    auto f = [nb](const float *p) { return p ? p + nb : nullptr; };
    auto b = [nb](const uint8_t *p) { return p ? p + nb : nullptr; };
    return {f(io.reward), f(io.value), f(io.last_value), f(io.tv), f(io.lb), f(io.lt), b(io.done), b(io.trunc), const_cast<float *>(f(io.out_a)), const_cast<float *>(f(io.out_b))};
}
template <int F, int O, int E>
__global__ void __launch_bounds__(WAVE, 4) k_gae(RetIo io, int64_t T, int64_t N, float gamma, float gl) {
    const int64_t nb = (int64_t)blockIdx.x * (WAVE * E);
    const uint32_t lo = threadIdx.x * E;
    if (nb + lo >= N) return;   // (with E > 1 the launcher has made sure that N is a multiple of E)
    ret_scan<F, false, O, E>(ret_block_io(io, nb), T, N, lo, gamma, gl, RgVtBars{});
}
template <int F, int O, int E>
__global__ void __launch_bounds__(WAVE, 4) k_vtrace(RetIo io, int64_t T, int64_t N, float gamma, float lam, RgVtBars bars) {
    const int64_t nb = (int64_t)blockIdx.x * (WAVE * E);
    const uint32_t lo = threadIdx.x * E;
    if (nb + lo >= N) return;
    ret_scan<F | RET_VALUE, true, O, E>(ret_block_io(io, nb), T, N, lo, gamma, lam, bars);
}

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launchers: defined here against the prototypes the host units call them by
// ---------------------------------------------------------------------------------------------
#ifndef RG_BUILD_ID
#define RG_BUILD_ID "unstamped"
#endif

// may a lane take E adjacent envs with one load per array?
static bool ret_wide_ok(const RetIo &io, int64_t N, int E) {
    if (E == 1) return true;
    if (N % E) return false;
    uintptr_t f = 0, b = 0;
    for (const float *p : {io.reward, io.value, io.last_value, io.tv, io.lb, io.lt, (const float *)io.out_a, (const float *)io.out_b}) f |= (uintptr_t)p;
    for (const uint8_t *p : {io.done, io.trunc}) b |= (uintptr_t)p;
    return !(f & (uintptr_t)(4 * E - 1)) && !(b & (uintptr_t)(E - 1));
}
template <bool VT, int F, int O, int E, class... A>
static void ret_launch_foe(const RetIo &io, int64_t T, int64_t N, hipStream_t st, const A &...args) {
    const dim3 grid((unsigned)((N + (int64_t)WAVE * E - 1) / ((int64_t)WAVE * E)));
    if constexpr (VT) rg_launch(k_vtrace<F, O, E>, grid, dim3(WAVE), 0, st, nullptr, nullptr, io, T, N, args...);
    else rg_launch(k_gae<F, O, E>, grid, dim3(WAVE), 0, st, nullptr, nullptr, io, T, N, args...);
}
template <bool VT, int F, int E, class... A>
static void ret_launch_fo(const RetIo &io, int64_t T, int64_t N, hipStream_t st, const A &...args) {
    if (io.out_a && io.out_b) ret_launch_foe<VT, F, 3, E>(io, T, N, st, args...);
    else if (io.out_a) ret_launch_foe<VT, F, 1, E>(io, T, N, st, args...);
    else ret_launch_foe<VT, F, 2, E>(io, T, N, st, args...);
}
template <bool VT, int F, class... A>
static void ret_launch_f(const RetIo &io, int64_t T, int64_t N, hipStream_t st, const A &...args) {
    if (RG_RET_ENVS > 1 && ret_wide_ok(io, N, RG_RET_ENVS)) ret_launch_fo<VT, F, RG_RET_ENVS>(io, T, N, st, args...);
    else ret_launch_fo<VT, F, 1>(io, T, N, st, args...);
}
// the instance that the present arrays name (trunc_value without trunc: refused by the caller)
template <bool VT, int V, class... A>
static void ret_launch_v(int f, const RetIo &io, int64_t T, int64_t N, hipStream_t st, const A &...args) {
    switch (f) {
#define RET_CASE(F) case F: ret_launch_f<VT, (F) | V>(io, T, N, st, args...); break;
        RET_CASE(0) RET_CASE(RET_DONE) RET_CASE(RET_TRUNC) RET_CASE(RET_DONE | RET_TRUNC) RET_CASE(RET_TRUNC | RET_TV) RET_CASE(RET_DONE | RET_TRUNC | RET_TV)
#undef RET_CASE
    }
}
template <bool VT, class... A>
static void ret_launch(const RetIo &io, int64_t T, int64_t N, hipStream_t st, const A &...args) {
    const int f = (io.done ? RET_DONE : 0) | (io.trunc ? RET_TRUNC : 0) | (io.trunc && io.tv ? RET_TV : 0);
    if constexpr (!VT) {   // (k_vtrace always has its value row: its F leaves the bit out)
        if (io.value) {
            ret_launch_v<VT, RET_VALUE>(f, io, T, N, st, args...);
            return;
        }
    }
    ret_launch_v<VT, 0>(f, io, T, N, st, args...);
}

extern "C" {
// the build id of this library, readable from the file as librogue_gym_hip.so's is (rg_api.cpp rg_build_id)
const char *rgk_returns_build_id(void) { static const char id[] = "RGBUILDID:" RG_BUILD_ID; return id + 10; }
// n_steps > 0, n_envs > 0 and every other argument checked by the caller (ret_args_check); gl = gamma * lam
void rgk_gae(int64_t n_steps, int64_t n_envs, const float *reward, const float *value, const float *last_value, const uint8_t *done, const uint8_t *trunc,
             const float *trunc_value, float gamma, float gl, float *adv, float *ret, hipStream_t st) {
    const RetIo io = {reward, value, last_value, trunc ? trunc_value : nullptr, nullptr, nullptr, done, trunc, adv, ret};
    ret_launch<false>(io, n_steps, n_envs, st, gamma, gl);
}
// bars: rho_bar, c_bar, pg_rho_bar and their logarithms
void rgk_vtrace(int64_t n_steps, int64_t n_envs, const float *logp_behaviour, const float *logp_target, const float *reward, const float *value, const float *last_value,
                const uint8_t *done, const uint8_t *trunc, const float *trunc_value, float gamma, float lam, const float *bars, float *vs, float *pg_adv, hipStream_t st) {
    const RetIo io = {reward, value, last_value, trunc ? trunc_value : nullptr, logp_behaviour, logp_target, done, trunc, vs, pg_adv};
    const RgVtBars b = {bars[0], bars[1], bars[2], bars[3], bars[4], bars[5]};
    ret_launch<true>(io, n_steps, n_envs, st, gamma, lam, b);
}
}
