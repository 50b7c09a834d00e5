// linalg_probe.hip — TEST HARNESS ONLY.  Calls the dense Newton-step factorisations and the wave primitives of the product headers
// (robogym_amd/csrc/rg_kernel.h, rb_kernel.h) AS THEY ARE, one workgroup per test matrix, at the block sizes the product launches them with,
// so that tests/test_linalg_kernels.py can hold them against float64 solves.  Built twice from this one source (Makefile): for gfx950
// (liblinalg_probe.so) and for the host emulation of the wavefront (liblinalg_probe_emul.so, -DRG_EMUL + tests/emul/hip_emul.cpp).
// The configurations are rg_api.hip's: rgs (rollout capacities) for the rg routines, rgl for the common namespace rb_kernel.h builds on,
// rgbs / rgbm (one wave) and rgb (four waves) for the rb routines.  Nothing here restates a routine: each kernel copies the inputs into
// the LDS fields and registers the routine reads, calls it, and copies back what it leaves.
#include "../../include/rgstep.h"
typedef rg_post_args RgPostArgs;
typedef rb_post_args RbPostArgs;
typedef ra_post_args RaPostArgs;
typedef ra_recipe_args RaRecipeArgs;
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "rg_types.h"
#include "rb_types.h"
#ifdef RG_EMUL
#include "hip_emul.h"
#else
#include <hip/hip_runtime.h>
#endif
// ------------------------------------------------------------------------------------------------- device memory and launches, both builds
#ifdef RG_EMUL
#define LP_AS4
static void* lp_alloc(size_t n) { return calloc(1, n ? n : 1); }
static void lp_free(void* p) { free(p); }
static void lp_h2d(void* d, const void* h, size_t n) { if (n) memcpy(d, h, n); }
static void lp_d2h(void* h, const void* d, size_t n) { if (n) memcpy(h, d, n); }
static int lp_sync() { return 0; }
#define LP_KERNEL(name, Args, body) static void name##_entry(void* p) { body(*(const Args*)p); }
#define LP_LAUNCH(name, nb, nt, lds, a) emul_launch_n((nb), (nt), (lds), name##_entry, (void*)&(a))
#else
#define LP_AS4 RG_AS4
static void* lp_alloc(size_t n) { void* p = 0; if (hipMalloc(&p, n ? n : 4) != hipSuccess) return 0; (void)hipMemset(p, 0, n ? n : 4); return p; }
static void lp_free(void* p) { (void)hipFree(p); }
static void lp_h2d(void* d, const void* h, size_t n) { if (n) (void)hipMemcpy(d, h, n, hipMemcpyHostToDevice); }
static void lp_d2h(void* h, const void* d, size_t n) { if (n) (void)hipMemcpy(h, d, n, hipMemcpyDeviceToHost); }
static int lp_sync() { return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess ? 0 : -1; }
#define LP_KERNEL(name, Args, body) __global__ void __launch_bounds__(256) name##_kernel(Args a) { body(a); }
#define LP_LAUNCH(name, nb, nt, lds, a) hipLaunchKernelGGL(name##_kernel, dim3(nb), dim3(nt), (lds), 0, (a))
#endif
// host buffers <-> device copies, freed at the end of a launcher
struct LpMem {
  std::vector<void*> ptr;
  template <class T> T* in(const T* h, size_t n) { T* d = (T*)lp_alloc(n * sizeof(T)); ptr.push_back(d); if (h) lp_h2d(d, h, n * sizeof(T)); return d; }
  template <class T> T* out(size_t n) { return in<T>((const T*)0, n); }
  ~LpMem() { for (void* p : ptr) lp_free(p); }
};

// ------------------------------------------------------------------------------------------------- rb: the group solves of rb_kernel.h
// rgbs / rgbm (one wave): rb_reg_solve (scaling, then rb_reg_solve_n<8/16/24/40/56> by the group's size).
// rgb (four waves): op 0 rb_scale_block + rb_chol_mfma + rb_group_solve (rb_chol_solve_wave); op 1 rb_scale_block + rb_chol + rb_chol_solve.
// The group's dofs are a permutation `perm` of 0 .. n-1 (b_group_dofs), right-hand side and solution indexed by dof.
struct LpRb { const RbModelDev* m; int op, n; const float* A; const float* g; float* x; float* Aout; float* sc; unsigned* ret; };
#define LP_RB_BODY(NS)                                                                                                                      \
  __device__ __forceinline__ void lp_##NS##_body(const LpRb& a) {                                                                          \
    using namespace NS;                                                                                                                     \
    RbM m = *(const LP_AS4 RbModelDev*)LP_UNI(a.m);                                                                                        \
    RbLds& s = RB_S();                                                                                                                      \
    const int b = blockIdx.x, n = a.n, nt = n * (n + 1) / 2;                                                                               \
    BFOR(w, nt) s.A[w] = a.A[(size_t)b * nt + w];                                                                                           \
    BFOR(d, n) s.grad[d] = a.g[(size_t)b * n + d];                                                                                          \
    BFOR(d, RB_MAXNV) s.search[d] = 0.f;                                                                                                    \
    BSYNC();                                                                                                                                \
    bool ok = true;                                                                                                                         \
    LP_RB_SOLVE(NS)                                                                                                                         \
    BFOR(d, n) a.x[(size_t)b * n + d] = s.search[d];                                                                                        \
    BFOR(w, nt) a.Aout[(size_t)b * nt + w] = s.A[w];                                                                                        \
    BFOR(l, n) a.sc[(size_t)b * n + l] = s.sc[l];                                                                                           \
    BSYNC();                                                                                                                                \
    if (TID == 0) a.ret[b] = ok ? 1u : 0u;                                                                                                  \
  }
#ifdef RG_EMUL
#define LP_UNI(p) (p)
#else
#define LP_UNI(p) rg_uniform(p)
#endif
#define RG_NS rgs
#define RG_MAXCON 24
#define RG_CPOOL 768
#define RG_MAXCAND 128
#define RG_MAXCAND2 64
#include "rg_kernel.h"
// ------------------------------------------------------------------------------------------------- rg: the dense Newton step of rg_kernel.h (configuration rgs)
// ops: 0 rg_chol_inv_solve_n<n> (then rg_cholinv_apply_n on g2), 1 rg_chol_mfma_n<n> (then rg_cholinv_apply_n on g2),
//      2 rg_chol<true> + rg_chol_solve_bwd (then rg_chol_solve on g2), 3 rg_chol<false> + rg_chol_solve on g,
//      4 rg_chol_inv_solve_n<n> of H, then rg_cholinv_woodbury_n<n> on g2 with the changed rows below (x2 = its result, ret = its return value)
struct LpRg {
  const RgModelDev* m; int op, n, hs;
  const float* H;      // [case][(n + 1) hs]: the work rows the routine reads (row n: the right-hand side g)
  const float* g2;     // [case][n]
  // op 4: static rows (slot r: desc, D, quad flags), pyramid rows (flags) and the contact / tendon tables they use (one case per launch)
  int ns, ncon; const int* sdesc; const float* sD; const int* squad; const int* pquad;
  const int* cdim; const int* cnnz; const int* coff; const int* cidx; const float* cD; const float* cmu; const float* cpool;
  const int* tcdof; const float* tenJ;
  float* x; float* x2; float* Hout; unsigned* st;   // st: status word, return value
};
__device__ __forceinline__ void lp_rg_body(const LpRg& a) {
  using namespace rgs;
  const RgModelDev* mp = a.m;
#ifdef RG_EMUL
  RgM m = *mp;
#else
  RgM m = *(const LP_AS4 RgModelDev*)rg_uniform(mp);
#endif
  RgLds& s = RG_S();
  const int b = blockIdx.x, n = a.n, hs = a.hs, rows = (n + 1) * hs;
  const float* Hin = a.H + (size_t)b * rows;
  for (int w = LANE; w < RG_HWORDS; w += RG_WAVE) s.H[w] = w < rows ? Hin[w] : 0.f;
  if (LANE == 0) { s.status = 0; s.ncon = a.op == 4 ? a.ncon : 0; }
  float* x = s.tmpv;
  PFOR(i, n) x[i] = Hin[n * hs + i];
  RowRegs R;
  if (a.op == 4) {
    PFOR(w, RG_MAXTEN * 4) { s.ten_cdof[w] = (unsigned char)a.tcdof[w]; s.tenJ[w] = a.tenJ[w]; }
    PFOR(c, a.ncon) { s.c_dim[c] = (unsigned char)a.cdim[c]; s.c_nnz[c] = (unsigned char)a.cnnz[c]; s.c_off[c] = (short)a.coff[c]; s.c_D[c] = a.cD[c]; s.c_mu[2 * c] = a.cmu[2 * c]; s.c_mu[2 * c + 1] = a.cmu[2 * c + 1]; }
    PFOR(w, a.ncon * RG_W) s.c_idx[w] = (unsigned char)a.cidx[w];
    PFOR(w, RG_CPOOL) s.c_pool[w] = a.cpool[w];
    PFOR(w, (int)sizeof(s.p_quad)) s.p_quad[w] = (unsigned char)(w < a.ncon * 6 ? a.pquad[w] : 0);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(R.desc) / sizeof(int)); k++) {
      const int r = LANE + RG_WAVE * k; const bool on = r < a.ns;
      R.desc[k] = on ? a.sdesc[r] : 0; R.D[k] = on ? a.sD[r] : 0.f; R.quad[k] = on ? a.squad[r] : 0;
    }
  }
  SYNC();
  unsigned ret = 1;
  if (a.op == 0 || a.op == 4) { if (n == 30) rg_chol_inv_solve_n<30>(m, s, x); else rg_chol_inv_solve_n<24>(m, s, x); }
  else if (a.op == 1) { if (n == 30) rg_chol_mfma_n<30>(m, s, x); else rg_chol_mfma_n<24>(m, s, x); }
  else if (a.op == 2) { rg_chol<true>(m, s); rg_chol_solve_bwd(m, s, x); }
  else { rg_chol<false>(m, s); rg_chol_solve(m, s, x); }
  PFOR(i, n) a.x[(size_t)b * n + i] = x[i];
  for (int w = LANE; w < rows; w += RG_WAVE) a.Hout[(size_t)b * rows + w] = s.H[w];
  SYNC();
  if (a.g2 && a.op != 3) {
    PFOR(i, n) x[i] = a.g2[(size_t)b * n + i];
    SYNC();
    if (a.op == 2) rg_chol_solve(m, s, x);
    else if (a.op == 4) { const bool ok = n == 30 ? rg_cholinv_woodbury_n<30>(m, s, R, x) : rg_cholinv_woodbury_n<24>(m, s, R, x); ret = ok ? 1u : 0u; }
    else if (n == 30) rg_cholinv_apply_n<30>(m, s, x); else rg_cholinv_apply_n<24>(m, s, x);
    PFOR(i, n) a.x2[(size_t)b * n + i] = x[i];
  }
  SYNC();
  if (LANE == 0) { a.st[2 * b] = s.status; a.st[2 * b + 1] = ret; }
}
LP_KERNEL(lp_rg, LpRg, lp_rg_body)

#undef RG_NS
#undef RG_MAXCON
#undef RG_CPOOL
#undef RG_MAXCAND
#undef RG_MAXCAND2
#define RG_NS rgl
#define RG_SETCONST 1
#define RG_MAXCON 64
#define RG_CPOOL 2048
#define RG_MAXCAND 256
#define RG_MAXCAND2 128
#include "rg_kernel.h"
#undef RG_NS
#undef RG_MAXCON
#undef RG_CPOOL
#undef RG_MAXCAND
#undef RG_MAXCAND2
#undef RG_SETCONST
#define RB_NS rgb
#define RB_T RB_T_LARGE
#define RB_MAXGROUP RB_MAXGROUP_LARGE
#define RB_MAXNV RB_MAXNV_LARGE
#define RB_MAXNQ RB_MAXNQ_LARGE
#define RB_WG_PER_CU 4
#include "rb_kernel.h"
#define LP_RB_SOLVE(NS)                                                                                                                     \
  rb_scale_block(s, n);                                                                                                                     \
  if (a.op == 0) { ok = rb_chol_mfma(s, n); rb_group_solve(m, s, 0, s.grad, s.search, 1.f); }                                              \
  else {                                                                                                                                    \
    ok = rb_chol(s, n);                                                                                                                     \
    BFOR(l, n) s.x[l] = s.sc[l] * s.grad[m.b_group_dofs[l]];                                                                               \
    BSYNC();                                                                                                                                \
    rb_chol_solve(s, n, s.x);                                                                                                               \
    BFOR(l, n) s.search[m.b_group_dofs[l]] = s.sc[l] * s.x[l];                                                                             \
    BSYNC();                                                                                                                                \
  }
LP_RB_BODY(rgb)
#undef LP_RB_SOLVE
LP_KERNEL(lp_rgb, LpRb, lp_rgb_body)
#undef RB_NS
#undef RB_T
#undef RB_MAXGROUP
#undef RB_MAXNV
#undef RB_MAXNQ
#undef RB_WG_PER_CU
#ifndef RB_CONW_ONEWAVE
#define RB_CONW_ONEWAVE 16
#endif
#undef RB_CONW
#define RB_CONW RB_CONW_ONEWAVE
#undef RB_MAXNU
#define RB_MAXNU 8
#define RB_NS rgbs
#define RB_T RB_T_SMALL
#define RB_MAXGROUP RB_MAXGROUP_SMALL
#define RB_MAXNV RB_MAXNV_SMALL
#define RB_MAXNQ RB_MAXNQ_SMALL
#define RB_WG_PER_CU 4
#include "rb_kernel.h"
#define LP_RB_SOLVE(NS) ok = rb_reg_solve(m, s, 0, s.grad, s.search, 1.f);
LP_RB_BODY(rgbs)
LP_KERNEL(lp_rgbs, LpRb, lp_rgbs_body)
#undef RB_NS
#undef RB_T
#undef RB_MAXGROUP
#undef RB_MAXNV
#undef RB_MAXNQ
#undef RB_WG_PER_CU
#define RB_NS rgbm
#define RB_T RB_T_MEDIUM
#define RB_MAXGROUP RB_MAXGROUP_MEDIUM
#define RB_MAXNV RB_MAXNV_MEDIUM
#define RB_MAXNQ RB_MAXNQ_MEDIUM
#define RB_WG_PER_CU 3
#include "rb_kernel.h"
LP_RB_BODY(rgbm)
#undef LP_RB_SOLVE
LP_KERNEL(lp_rgbm, LpRb, lp_rgbm_body)
#undef RB_NS
#undef RB_T
#undef RB_MAXGROUP
#undef RB_MAXNV
#undef RB_MAXNQ
#undef RB_WG_PER_CU

// ------------------------------------------------------------------------------------------------- wave primitives (rg_kernel.h's common part)
// out (floats, per lane): [0] wave_sum(v) [1] wave_max(v) [2] argmax value [3..6] grp_max<2,4,8,16>(v) [7] grp_sum16(v) [8..9] rg_halves<0/1>(v, u)
//                         [10 .. 73] lane_bcast(v, src) for src = 0..63 [74 .. 89] rg_mfma32 chain of K steps (A: fa[k][lane], B: fb[k][lane])
// iout (ints, per lane):  [0] wave_min_i(iv) [1] argmax index [2..5] grp_min_i<2,4,8,16>(iv)
// fx -> fo: rg_rcp, rg_rsqrt, rg_sqrt of nf numbers (lane-strided)
#define LP_CPOOL ((int)(sizeof(rgs::RgLds::c_pool) / sizeof(float)))
#define LP_NOUT 90
#define LP_NIOUT 6
struct LpPrim { const float* v; const float* u; const int* iv; const int* ix; int K; const float* fa; const float* fb; int nf; const float* fx; float* out; int* iout; float* fo; };
__device__ __forceinline__ void lp_prim_body(const LpPrim& a) {
  const int l = LANE;
  const float v = a.v[l], u = a.u[l]; const int iv = a.iv[l];
  float* o = a.out + (size_t)l * LP_NOUT; int* io = a.iout + (size_t)l * LP_NIOUT;
  o[0] = wave_sum(v);
  o[1] = wave_max(v);
  io[0] = wave_min_i(iv);
  float av = v; int ai = a.ix[l]; wave_argmax(av, ai); o[2] = av; io[1] = ai;
  o[3] = grp_max<2>(v); o[4] = grp_max<4>(v); o[5] = grp_max<8>(v); o[6] = grp_max<16>(v);
  io[2] = grp_min_i<2>(iv); io[3] = grp_min_i<4>(iv); io[4] = grp_min_i<8>(iv); io[5] = grp_min_i<16>(iv);
  o[7] = grp_sum16(v);
  o[8] = rg_halves<0>(v, u); o[9] = rg_halves<1>(v, u);
  for (int src = 0; src < 64; src++) o[10 + src] = lane_bcast(v, src);
  rgacc acc;
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  for (int k = 0; k < a.K; k++) rg_mfma32(a.fa[64 * k + l], a.fb[64 * k + l], acc);
  for (int r = 0; r < 16; r++) o[74 + r] = acc[r];
  for (int w = l; w < a.nf; w += RG_WAVE) { const float xx = a.fx[w]; a.fo[3 * w] = rg_rcp(xx); a.fo[3 * w + 1] = rg_rsqrt(xx); a.fo[3 * w + 2] = rg_sqrt(xx); }
}
LP_KERNEL(lp_prim, LpPrim, lp_prim_body)

// ------------------------------------------------------------------------------------------------- C ABI (host arrays in, host arrays out; 0 = ok)
extern "C" {
int lp_rg_lds_words() { return RG_HWORDS; }
int lp_rg_limits(int* out) { out[0] = RG_HWORDS; out[1] = RG_MAXNVC; out[2] = RG_WOODBURY; out[3] = RG_MAXSROW; out[4] = RG_MAXTEN; out[5] = 24; out[6] = LP_CPOOL; out[7] = RG_W; return 0; }
int lp_rb_limits(int* out) { out[0] = RB_MAXGROUP_SMALL; out[1] = RB_MAXGROUP_MEDIUM; out[2] = RB_MAXGROUP_LARGE; out[3] = RB_MAXNV_SMALL; out[4] = RB_MAXNV_MEDIUM; out[5] = RB_MAXNV_LARGE; return 0; }

// nb cases of size n; g2 may be null.  Woodbury (op 4): nb = 1, the row tables as described at LpRg.
int lp_rg(int op, int n, int nb, const float* H, const float* g2, int ns, const int* sdesc, const float* sD, const int* squad, int ncon, const int* pquad,
          const int* cdim, const int* cnnz, const int* coff, const int* cidx, const float* cD, const float* cmu, const float* cpool, const int* tcdof, const float* tenJ,
          float* x, float* x2, float* Hout, unsigned* st) {
  using namespace rgs;
  const int hs = (n + 3) / 4 * 4;
  if (n < 1 || n > RG_MAXNVC || (n + 1) * hs > RG_HWORDS || nb < 1 || op < 0 || op > 4) return -2;
  if ((op == 0 || op == 1 || op == 4) && n != 24 && n != 30) return -2;
  if (op == 4 && (nb != 1 || ns > RG_MAXSROW || ncon > 24 || !g2)) return -2;
  RgModelDev md; memset(&md, 0, sizeof md);
  md.nvc = n; md.hs = hs; md.nfric_dof = op == 4 ? ns : 0;
  LpMem M;
  LpRg a; memset(&a, 0, sizeof a);
  a.m = M.in(&md, 1); a.op = op; a.n = n; a.hs = hs;
  a.H = M.in(H, (size_t)nb * (n + 1) * hs);
  a.g2 = g2 ? M.in(g2, (size_t)nb * n) : 0;
  if (op == 4) {
    std::vector<int> z(RG_MAXTEN * 4, 255); std::vector<float> zf(RG_MAXTEN * 4, 0.f), zp(LP_CPOOL, 0.f);
    a.ns = ns; a.ncon = ncon;
    a.sdesc = M.in(sdesc, ns); a.sD = M.in(sD, ns); a.squad = M.in(squad, ns);
    a.pquad = M.in(pquad, ncon * 6); a.cdim = M.in(cdim, ncon); a.cnnz = M.in(cnnz, ncon); a.coff = M.in(coff, ncon); a.cidx = M.in(cidx, (size_t)ncon * RG_W);
    a.cD = M.in(cD, ncon); a.cmu = M.in(cmu, 2 * ncon); a.cpool = M.in(cpool ? cpool : zp.data(), LP_CPOOL);
    a.tcdof = M.in(tcdof ? tcdof : z.data(), RG_MAXTEN * 4); a.tenJ = M.in(tenJ ? tenJ : zf.data(), RG_MAXTEN * 4);
  }
  a.x = M.out<float>((size_t)nb * n); a.x2 = M.out<float>((size_t)nb * n); a.Hout = M.out<float>((size_t)nb * (n + 1) * hs); a.st = M.out<unsigned>(2 * (size_t)nb);
  LP_LAUNCH(lp_rg, nb, RG_WAVE, sizeof(RgLds), a);
  if (lp_sync()) return -1;
  lp_d2h(x, a.x, sizeof(float) * nb * n); if (x2) lp_d2h(x2, a.x2, sizeof(float) * nb * n);
  lp_d2h(Hout, a.Hout, sizeof(float) * nb * (n + 1) * hs); lp_d2h(st, a.st, sizeof(unsigned) * 2 * nb);
  return 0;
}

// cfg 0: rgbs, 1: rgbm, 2: rgb (op 0 matrix pipe, op 1 LDS path).  A: nb packed lower triangles; g, x: [nb][n] by dof; perm: b_group_dofs
int lp_rb(int cfg, int op, int n, int nb, const float* A, const float* g, const int* perm, float* x, float* Aout, float* sc, unsigned* ret) {
  const int cap = cfg == 0 ? RB_MAXGROUP_SMALL : (cfg == 1 ? RB_MAXGROUP_MEDIUM : RB_MAXGROUP_LARGE);
  const int nvcap = cfg == 0 ? RB_MAXNV_SMALL : (cfg == 1 ? RB_MAXNV_MEDIUM : RB_MAXNV_LARGE);
  if (n < 1 || n > cap || n > nvcap || nb < 1 || cfg < 0 || cfg > 2) return -2;
  for (int l = 0; l < n; l++) if (perm[l] < 0 || perm[l] >= n) return -2;
  const int nt = n * (n + 1) / 2;
  RbModelDev md; memset(&md, 0, sizeof md);
  LpMem M;
  const int adr[2] = {0, n};
  md.nv = n; md.ngroup = 1; md.gmax = n;
  md.b_group_adr = M.in(adr, 2); md.b_group_dofs = M.in(perm, n);
  LpRb a; memset(&a, 0, sizeof a);
  a.m = M.in(&md, 1); a.op = op; a.n = n;
  a.A = M.in(A, (size_t)nb * nt); a.g = M.in(g, (size_t)nb * n);
  a.x = M.out<float>((size_t)nb * n); a.Aout = M.out<float>((size_t)nb * nt); a.sc = M.out<float>((size_t)nb * n); a.ret = M.out<unsigned>(nb);
  if (cfg == 0) LP_LAUNCH(lp_rgbs, nb, RB_T_SMALL, sizeof(rgbs::RbLds), a);
  else if (cfg == 1) LP_LAUNCH(lp_rgbm, nb, RB_T_MEDIUM, sizeof(rgbm::RbLds), a);
  else LP_LAUNCH(lp_rgb, nb, RB_T_LARGE, sizeof(rgb::RbLds), a);
  if (lp_sync()) return -1;
  lp_d2h(x, a.x, sizeof(float) * nb * n); lp_d2h(Aout, a.Aout, sizeof(float) * nb * nt); lp_d2h(sc, a.sc, sizeof(float) * nb * n); lp_d2h(ret, a.ret, sizeof(unsigned) * nb);
  return 0;
}

int lp_prim(const float* v, const float* u, const int* iv, const int* ix, int K, const float* fa, const float* fb, int nf, const float* fx, float* out, int* iout, float* fo) {
  if (K < 0 || K > 64 || nf < 0) return -2;
  LpMem M;
  LpPrim a;
  a.v = M.in(v, 64); a.u = M.in(u, 64); a.iv = M.in(iv, 64); a.ix = M.in(ix, 64); a.K = K;
  a.fa = M.in(fa, 64 * (size_t)(K ? K : 1)); a.fb = M.in(fb, 64 * (size_t)(K ? K : 1));
  a.nf = nf; a.fx = M.in(fx, nf ? nf : 1);
  a.out = M.out<float>(64 * LP_NOUT); a.iout = M.out<int>(64 * LP_NIOUT); a.fo = M.out<float>(3 * (size_t)(nf ? nf : 1));
  LP_LAUNCH(lp_prim, 1, 64, 16, a);
  if (lp_sync()) return -1;
  lp_d2h(out, a.out, sizeof(float) * 64 * LP_NOUT); lp_d2h(iout, a.iout, sizeof(int) * 64 * LP_NIOUT); lp_d2h(fo, a.fo, sizeof(float) * 3 * nf);
  return 0;
}
}
