// K16: forward-backward of an input-driven HMM (IO-HMM) with a transition matrix per (time step, chain), in log space
// (ref models/dHMM.py:42-78).  One launch replaces the reference's two Python loops over T.
// Layout as K11 (k_hmm.hip): a chain is owned by Kp lanes (Kp = K padded to a power of two), lane j owns target state
// j -- column j of the step's transition matrix in registers, entry j of the message; K-vectors that every lane must see
// and the K x K pair weights (written by columns, summed by rows) go through a small per-chain LDS buffer, scalar
// reductions through DPP butterflies.  Unlike K11 the transition matrix changes at every step, so K11's factorisation
// with exp(tr) kept in registers does not apply: every step is the literal log-space step with ONE exponential per
// (source, target) pair.  The per-step operands do not depend on the recursion and are requested one step ahead.
// The pair posterior of every step is written out (the gate's M-step regresses it on the step's input).  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vbmp_dispatch.h"
#include "../../include/vbmp_hip.h"

namespace vbmp {
namespace dhmm {

// wave-level LDS ordering (LDS address space only)
__device__ __forceinline__ void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// xor butterfly over the Kp lanes of a chain: DPP moves inside a 16-lane row, ds_bpermute across rows (see k_hmm.hip)
template <int CTRL>
__device__ __forceinline__ float dpp_xchg(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ double dpp_xchg(double v) {
  union { double d; int i[2]; } a, r;
  a.d = v;
  r.i[0] = __builtin_amdgcn_update_dpp(0, a.i[0], CTRL, 0xf, 0xf, true);
  r.i[1] = __builtin_amdgcn_update_dpp(0, a.i[1], CTRL, 0xf, 0xf, true);
  return r.d;
}
template <int Kp, typename T, typename F>
__device__ __forceinline__ T grp_butterfly(T v, F op) {
  if constexpr (Kp >= 2) v = op(v, dpp_xchg<0xB1>(v));   // quad_perm:[1,0,3,2]  (lane ^ 1)
  if constexpr (Kp >= 4) v = op(v, dpp_xchg<0x4E>(v));   // quad_perm:[2,3,0,1]  (lane ^ 2)
  if constexpr (Kp >= 8) v = op(v, dpp_xchg<0x141>(v));  // row_half_mirror
  if constexpr (Kp >= 16) v = op(v, dpp_xchg<0x140>(v)); // row_mirror
  if constexpr (Kp >= 32) v = op(v, __shfl_xor(v, 16, 64));
  if constexpr (Kp >= 64) v = op(v, __shfl_xor(v, 32, 64));
  return v;
}
template <int Kp, typename T>
__device__ __forceinline__ T grp_max(T v) {
  return grp_butterfly<Kp>(v, [](T a, T b) { return b > a ? b : a; });
}
template <int Kp, typename T>
__device__ __forceinline__ T grp_sum(T v) {
  return grp_butterfly<Kp>(v, [](T a, T b) { return a + b; });
}

// smallest row sum of pair weights whose log is taken as it stands (below it a row is redone in log space)
template <typename T> __device__ __forceinline__ T row_tiny();
template <> __device__ __forceinline__ double row_tiny<double>() { return 1e-290; }
template <> __device__ __forceinline__ float row_tiny<float>() { return 1e-30f; }

// NaN conventions follow the reference's stable_logsumexp (max + log sum exp(x - max)): a log-sum-exp over a set whose
// maximum is -inf is NaN, and a NaN anywhere in the set makes it NaN (exp(NaN - m) enters the sum).
template <typename T, int Kp>
__global__ __launch_bounds__(64) void k_dhmm_fb(const T* __restrict__ obs, const T* __restrict__ tr,
                                                const T* __restrict__ init, int64_t Tn, int64_t C, int64_t NB, int K,
                                                T ptemp, T* __restrict__ p, T* __restrict__ SEzz, T* __restrict__ SEz0,
                                                T* __restrict__ logZ) {
  constexpr int CPW = 64 / Kp;  // chains per wave
  constexpr int LDM = Kp + 1;   // odd row stride of the pair weights: lane j reads ROW j
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* smem = reinterpret_cast<T*>(smem_raw);
  const int lane = threadIdx.x, cl = lane / Kp, j = lane % Kp;
  const int64_t c = (int64_t)blockIdx.x * CPW + cl;
  const bool live = (c < C) && (j < K);
  const bool on = j < K;
  const int64_t cc = c < C ? c : C - 1;
  const int jj = on ? j : 0;
  T* vec = smem + cl * (3 * Kp + Kp * LDM);  // [Kp] source message, [Kp] + [Kp] column quantities, [Kp][LDM] pair weights
  T* aux = vec + Kp;
  T* aux2 = aux + Kp;
  T* mat = aux2 + Kp;
  const T NI = -INFINITY, QN = T(NAN);
  const int64_t ts = C * K, tts = C * K * K;
  const T* ob = obs + cc * K + jj;          // element (t, c, j) at ob[t*ts]
  const T* trj = tr + cc * K * K + jj;      // element (t, c, i, j) at trj[t*tts + i*K]
  T* pj = p + cc * K + jj;
  T* zj = SEzz + cc * K * K + jj;
  const T in_j = on ? init[(cc % NB) * K + j] : NI;

  T trc[Kp], trn[Kp];
  auto load_col = [&](int64_t t) {
#pragma unroll
    for (int i = 0; i < Kp; ++i) trn[i] = (i < K) ? trj[t * tts + (int64_t)i * K] : NI;
  };

  // ---------------------------------------------------------------- forward (:47-52)
  // f[0]_j = lse_i((obs[0]_j + init_i) + tr[0]_ij),  f[t]_j = lse_i((f[t-1]_i + obs[t]_j) + tr[t]_ij)
  T prev = in_j;
  load_col(0);
  T o_next = ob[0];
  for (int64_t t = 0; t < Tn; ++t) {
#pragma unroll
    for (int i = 0; i < Kp; ++i) trc[i] = trn[i];
    const T o = o_next;
    // the operands of step t+1 are requested at the top of step t
    const int64_t tn = (t + 1 < Tn) ? t + 1 : t;
    load_col(tn);
    o_next = ob[tn * ts];
    wsync();  // the previous readers of vec are done
    vec[j] = prev;
    wsync();
    T m = NI;
#pragma unroll
    for (int i = 0; i < Kp; ++i)
      if (i < K) {
        const T v = (vec[i] + o) + trc[i];
        m = v > m ? v : m;
      }
    T s = T(0);
#pragma unroll
    for (int i = 0; i < Kp; ++i)
      if (i < K) s += exp(((vec[i] + o) + trc[i]) - m);
    prev = on ? ((m > NI) ? m + log(s) : QN) : NI;
    if (live) pj[t * ts] = prev;  // the p buffer holds the filtered logits until the backward sweep
  }

  // logZ = lse_j f[T-1]_j (:53-55)
  T lz;
  {
    const T m = grp_max<Kp>(prev);
    const T s = grp_sum<Kp>(on ? exp(prev - m) : T(0));
    lz = (m > NI) ? m + log(s) : QN;
  }
  // softmax of a message held one entry per lane, with temperature (:72-73)
  auto soft = [&](T mine, T temp) -> T {
    const T mx = grp_max<Kp>(on ? mine : NI);
    const T e = on ? exp((mine - mx) / temp) : T(0);
    return e / grp_sum<Kp>(e);
  };
  T nxt = on ? prev - lz : NI;  // smoothed (= filtered) message at T-1
  {
    const T pt = soft(nxt, ptemp);
    if (live) pj[(Tn - 1) * ts] = pt;
  }

  // ---------------------------------------------------------------- backward smoothing (:57-70)
  // with x = the normalised filtered message at t (the initial distribution for t = -1) and s = the smoothed one at t+1:
  //   xi_ij = ((x_i + tr[t+1]_ij) - c_j) + s_j,  c_j = lse_i(x_i + tr[t+1]_ij)
  //   s[t]_i = lse_j xi_ij,   SEzz[t+1] = softmax_ij xi
  // Lane j takes its column's maximum m_j and weights w_ij = exp(x_i + tr_ij - m_j) (the one exponential per pair), so
  // that c_j = m_j + log S_j (S_j = sum_i w_ij) and exp(xi_ij - G) = w_ij u_j with u_j = exp(s_j - G) / S_j,
  // G = max_j s_j: every weight <= 1 and the total sum_ij >= 1/K.  Row i's sum r_i gives s[t]_i = G + log r_i unless it
  // is below row_tiny (the row's pairs all sit far below G, or all are forbidden): that row is redone literally in log
  // space, which also yields the reference's NaN for a row of -inf.
  load_col(Tn - 1);
  T f_next = (Tn >= 2) ? pj[(Tn - 2) * ts] : T(0);
  for (int64_t t = Tn - 2; t >= -1; --t) {
#pragma unroll
    for (int i = 0; i < Kp; ++i) trc[i] = trn[i];  // tr[t+1]
    const T flt = f_next;
    // tr[t] and the filtered logits of step t-1 are requested at the top of step t (the step writes slot t of p only)
    load_col(t >= 0 ? t : 0);
    f_next = pj[(t >= 1 ? t - 1 : 0) * ts];
    const T x = on ? ((t >= 0) ? flt - lz : in_j) : NI;
    wsync();  // the previous readers of vec / aux / mat are done
    vec[j] = x;
    wsync();
    T m = NI;
#pragma unroll
    for (int i = 0; i < Kp; ++i)
      if (i < K) {
        const T v = vec[i] + trc[i];
        m = v > m ? v : m;
      }
    T S = T(0);
#pragma unroll
    for (int i = 0; i < Kp; ++i)
      if (i < K) {
        const T w = exp((vec[i] + trc[i]) - m);
        mat[i * LDM + j] = w;
        S += w;
      }
    const T G = grp_max<Kp>(nxt);
    // a column that no source reaches has c_j = NaN in the reference, and so has every xi of the column
    const T u = on ? ((m > NI) ? exp(nxt - G) / S : QN) : T(0);
    aux[j] = u;
    wsync();
    T r = T(0);  // row j of the weights: unnormalised smoothed posterior of state j at the source time
#pragma unroll
    for (int k = 0; k < Kp; ++k)
      if (k < K) r += mat[j * LDM + k] * aux[k];
    const T total = grp_sum<Kp>(on ? r : T(0));
    T s_new = on ? G + log(r) : NI;
    const bool redo = on && !(r >= row_tiny<T>());
    if (__ballot(redo)) {  // wave-uniform: rare
      wsync();
      aux[j] = on ? ((m > NI) ? m + log(S) : QN) : T(0);  // c_j
      aux2[j] = nxt;                                      // s_j
      wsync();
      if (redo) {
        const T* row = tr + ((t + 1) * C + cc) * K * K + (int64_t)j * K;  // row j of tr[t+1]
        T m2 = NI;
        for (int k = 0; k < K; ++k) {
          const T v = ((x + row[k]) - aux[k]) + aux2[k];
          m2 = v > m2 ? v : m2;
        }
        T s2 = T(0);
        for (int k = 0; k < K; ++k) s2 += exp((((x + row[k]) - aux[k]) + aux2[k]) - m2);
        s_new = (m2 > NI) ? m2 + log(s2) : QN;
      }
    }
    if (live) {
      const T sc = u / total;
#pragma unroll
      for (int i = 0; i < Kp; ++i)
        if (i < K) zj[(t + 1) * tts + (int64_t)i * K] = mat[i * LDM + j] * sc;
    }
    nxt = s_new;
    if (t >= 0) {
      const T pt = soft(nxt, ptemp);
      if (live) pj[t * ts] = pt;
    } else {
      const T pz = soft(nxt, T(1));  // posterior of the virtual state before step 0 (:65-66)
      if (live) SEz0[cc * K + j] = pz;
    }
  }
  if (live && j == 0) logZ[cc] = lz;
}

template <typename T, int Kp>
static int launch_dhmm(const T* obs, const T* tr, const T* init, int64_t Tn, int64_t C, int64_t NB, int K, T ptemp, T* p,
                       T* SEzz, T* SEz0, T* logZ, hipStream_t st) {
  constexpr int CPW = 64 / Kp;
  const int64_t blocks = (C + CPW - 1) / CPW;
  const size_t smem = (size_t)CPW * (3 * Kp + Kp * (Kp + 1)) * sizeof(T);
  hipLaunchKernelGGL((k_dhmm_fb<T, Kp>), dim3((unsigned)blocks), dim3(64), smem, st, obs, tr, init, Tn, C, NB, K, ptemp,
                     p, SEzz, SEz0, logZ);
  return hipGetLastError() == hipSuccess ? 0 : VBMP_ERR_LAUNCH;
}

template <typename T>
static int dhmm_dispatch(const T* obs, const T* tr, const T* init, int64_t Tn, int64_t C, int64_t NB, int K, T ptemp,
                         T* p, T* SEzz, T* SEz0, T* logZ, void* stream) {
  if (Tn < 0 || C < 0 || NB < 0 || K < 1 || K > VBMP_DHMM_MAX_K) return VBMP_ERR_ARG;
  if (Tn == 0 || C == 0) return 0;
  if (!obs || !tr || !init || !p || !SEzz || !SEz0 || !logZ || NB < 1) return VBMP_ERR_ARG;
  if (C > ((int64_t)1 << 31)) return VBMP_ERR_ARG;  // grid.x
  hipStream_t st = (hipStream_t)stream;
  if (K <= 2) return launch_dhmm<T, 2>(obs, tr, init, Tn, C, NB, K, ptemp, p, SEzz, SEz0, logZ, st);
  if (K <= 4) return launch_dhmm<T, 4>(obs, tr, init, Tn, C, NB, K, ptemp, p, SEzz, SEz0, logZ, st);
  if (K <= 8) return launch_dhmm<T, 8>(obs, tr, init, Tn, C, NB, K, ptemp, p, SEzz, SEz0, logZ, st);
  if (K <= 16) return launch_dhmm<T, 16>(obs, tr, init, Tn, C, NB, K, ptemp, p, SEzz, SEz0, logZ, st);
  if (K <= 32) return launch_dhmm<T, 32>(obs, tr, init, Tn, C, NB, K, ptemp, p, SEzz, SEz0, logZ, st);
  return launch_dhmm<T, 64>(obs, tr, init, Tn, C, NB, K, ptemp, p, SEzz, SEz0, logZ, st);
}

}  // namespace dhmm
}  // namespace vbmp

extern "C" {
int vbmp_dhmm_forward_backward_f64(const double* obs, const double* tr, const double* init, int64_t Tn, int64_t C,
                                   int64_t NB, int K, double ptemp, double* p, double* SEzz, double* SEz0, double* logZ,
                                   void* stream) {
  return vbmp::dhmm::dhmm_dispatch<double>(obs, tr, init, Tn, C, NB, K, ptemp, p, SEzz, SEz0, logZ, stream);
}
int vbmp_dhmm_forward_backward_f32(const float* obs, const float* tr, const float* init, int64_t Tn, int64_t C,
                                   int64_t NB, int K, float ptemp, float* p, float* SEzz, float* SEz0, float* logZ,
                                   void* stream) {
  return vbmp::dhmm::dhmm_dispatch<float>(obs, tr, init, Tn, C, NB, K, ptemp, p, SEzz, SEz0, logZ, stream);
}
}
