// mb_chain.hip -- ticks per DP step of the SW-linear pass-1 recurrence (G-space, no floor) when the
// cell above is taken inside the max (v_max_i32_dpp) instead of by a v_mov_b32_dpp in front of the
// v_max3.  One lone wave, and four waves on four SIMDs.  Diagnostic only.
//   0 (a)  R = 2 today: DPP -> v_max3 (row 1) -> v_max3 (row 2), as flow_kernel compiles it
//   1 (b)  R = 2 fused, per-lane neutral input (lanes >= 1 hold MSA_NEG where lane 0 holds the ring
//          value): t = max3(U + s, X, IN*) off the chain, h1 = max(dpp(X2), t), h2 = max3(b, h1, X2)
//   2 (b') the same with the two profile v_perm of the next four steps in two of the four filler slots
//   3 (c)  R = 2 fused, the ring value in every lane: one more off-chain v_max (t without IN as the
//          DPP op's src1, t with IN as its destination's content)
//   4      R = 1 today: DPP -> v_max3
//   7 (b2) (b) in the order t, b, U', h1, a', h2: both DPP ops sit two instructions behind the writes
//          of their operands with no filler, and no instruction reads the result of the one before it
//   8 (a*) today's five instructions hand-ordered a, b, DPP, h1, h2: the two adds fill the DPP's wait states
//          in every step (the compiler's order leaves an s_nop in about every third step)
//   6 (a+) control: (a) plus one VALU per step that nothing depends on (issue-bound or chain-bound?)
//   5 (d)  R = 1 fused: t = max(U + s, IN*), m = max(dpp(X), t), h = max(m, X)
// A DPP op reads a VGPR no sooner than two wait states after the VALU that wrote it, and nothing pads
// an asm string, so every fused step is one hand-ordered block with its filler slot.
#include <hip/hip_runtime.h>
#include <cstdio>

#define NEG (-(1 << 28))
__device__ __forceinline__ int dpp_shr1(int old, int src) { return __builtin_amdgcn_update_dpp(old, src, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int imax3(int a, int b, int c) { return max(max(a, b), c); }

#define DPPC " wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"
#define SDWA(sel) " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_" #sel "\n\t"

// (b): in: a = U + s of this step, X, X2, IN* ; out: X = h1, X2 = h2, IN = the next diagonal, a = the
// next step's U + s (byte SELN of swn)
#define STEP_B(SELB, SELN, FILL)                                                                      \
  asm volatile("v_max3_i32 %[t], %[a], %[x], %[in]\n\t"                                               \
               "v_add_u32_sdwa %[b], %[x], sext(%[swb])" SDWA(SELB)                                   \
               FILL                                                                                   \
               "v_max_i32_dpp %[t], %[x2], %[t]" DPPC                                                 \
               "v_mov_b32_dpp %[in], %[x2]" DPPC                                                      \
               "v_add_u32_sdwa %[an], %[in], sext(%[swn])" SDWA(SELN)                                 \
               "v_max3_i32 %[h2], %[b], %[t], %[x2]"                                                  \
               : [t] "=&v"(t), [b] "=&v"(b), [in] "+v"(in), [an] "=&v"(an), [h2] "=&v"(h2)           \
               : [a] "v"(a), [x] "v"(X), [x2] "v"(X2), [swb] "v"(swb), [swn] "v"(swn))

template <int KK, int FILL>
__device__ __forceinline__ void step_b(int& a, int& X, int& X2, int& in, unsigned swb, unsigned swn, unsigned& pa,
                                       unsigned plo, unsigned phi, unsigned cwn) {
  int t, b, an, h2;
  if constexpr (FILL == 1) {  // filler: a profile v_perm of the next four steps
    asm volatile("v_max3_i32 %[t], %[a], %[x], %[in]\n\t"
                 "v_add_u32_sdwa %[b], %[x], sext(%[swb])" SDWA(0)
                 "v_perm_b32 %[pa], %[phi], %[plo], %[cwn]\n\t"
                 "v_max_i32_dpp %[t], %[x2], %[t]" DPPC
                 "v_mov_b32_dpp %[in], %[x2]" DPPC
                 "v_add_u32_sdwa %[an], %[in], sext(%[swn])" SDWA(1)
                 "v_max3_i32 %[h2], %[b], %[t], %[x2]"
                 : [t] "=&v"(t), [b] "=&v"(b), [in] "+v"(in), [an] "=&v"(an), [h2] "=&v"(h2), [pa] "=&v"(pa)
                 : [a] "v"(a), [x] "v"(X), [x2] "v"(X2), [swb] "v"(swb), [swn] "v"(swn), [phi] "v"(phi), [plo] "v"(plo),
                   [cwn] "v"(cwn));
  } else if constexpr (FILL == 2) {
    asm volatile("v_max3_i32 %[t], %[a], %[x], %[in]\n\t"
                 "v_add_u32_sdwa %[b], %[x], sext(%[swb])" SDWA(1)
                 "v_perm_b32 %[pa], %[phi], %[plo], %[cwn]\n\t"
                 "v_max_i32_dpp %[t], %[x2], %[t]" DPPC
                 "v_mov_b32_dpp %[in], %[x2]" DPPC
                 "v_add_u32_sdwa %[an], %[in], sext(%[swn])" SDWA(2)
                 "v_max3_i32 %[h2], %[b], %[t], %[x2]"
                 : [t] "=&v"(t), [b] "=&v"(b), [in] "+v"(in), [an] "=&v"(an), [h2] "=&v"(h2), [pa] "=&v"(pa)
                 : [a] "v"(a), [x] "v"(X), [x2] "v"(X2), [swb] "v"(swb), [swn] "v"(swn), [phi] "v"(phi), [plo] "v"(plo),
                   [cwn] "v"(cwn));
  } else if constexpr (KK == 0) STEP_B(0, 1, "s_nop 0\n\t");
  else if constexpr (KK == 1) STEP_B(1, 2, "s_nop 0\n\t");
  else if constexpr (KK == 2) STEP_B(2, 3, "s_nop 0\n\t");
  else STEP_B(3, 0, "s_nop 0\n\t");
  a = an;
  X = t;
  X2 = h2;
}

// (a*): today's step as one ordered block.  in: U (the diagonal), X, X2, IN; out: X = h1, X2 = h2, IN = up
#define STEP_A(SEL)                                                                                   \
  asm volatile("v_add_u32_sdwa %[a], %[u], sext(%[sw])" SDWA(SEL)                                     \
               "v_add_u32_sdwa %[b], %[x], sext(%[swb])" SDWA(SEL)                                    \
               "v_mov_b32_dpp %[in], %[x2]" DPPC                                                      \
               "v_max3_i32 %[h1], %[a], %[in], %[x]\n\t"                                              \
               "v_max3_i32 %[h2], %[b], %[h1], %[x2]"                                                 \
               : [a] "=&v"(a), [b] "=&v"(b), [in] "+v"(in), [h1] "=&v"(h1), [h2] "=&v"(h2)           \
               : [u] "v"(U), [x] "v"(X), [x2] "v"(X2), [sw] "v"(sw), [swb] "v"(swb))

template <int KK>
__device__ __forceinline__ void step_a(int& U, int& X, int& X2, int& in, unsigned sw, unsigned swb) {
  int a, b, h1, h2;
  if constexpr (KK == 0) STEP_A(0);
  else if constexpr (KK == 1) STEP_A(1);
  else if constexpr (KK == 2) STEP_A(2);
  else STEP_A(3);
  U = in;
  X = h1;
  X2 = h2;
}

// (b2): the same six instructions with the diagonal's DPP in front of the fused max -- no filler slot
#define STEP_B2(SELB, SELN)                                                                           \
  asm volatile("v_max3_i32 %[t], %[a], %[x], %[in]\n\t"                                               \
               "v_add_u32_sdwa %[b], %[x], sext(%[swb])" SDWA(SELB)                                   \
               "v_mov_b32_dpp %[in], %[x2]" DPPC                                                      \
               "v_max_i32_dpp %[t], %[x2], %[t]" DPPC                                                 \
               "v_add_u32_sdwa %[an], %[in], sext(%[swn])" SDWA(SELN)                                 \
               "v_max3_i32 %[h2], %[b], %[t], %[x2]"                                                  \
               : [t] "=&v"(t), [b] "=&v"(b), [in] "+v"(in), [an] "=&v"(an), [h2] "=&v"(h2)           \
               : [a] "v"(a), [x] "v"(X), [x2] "v"(X2), [swb] "v"(swb), [swn] "v"(swn))

template <int KK>
__device__ __forceinline__ void step_b2(int& a, int& X, int& X2, int& in, unsigned swb, unsigned swn) {
  int t, b, an, h2;
  if constexpr (KK == 0) STEP_B2(0, 1);
  else if constexpr (KK == 1) STEP_B2(1, 2);
  else if constexpr (KK == 2) STEP_B2(2, 3);
  else STEP_B2(3, 0);
  a = an;
  X = t;
  X2 = h2;
}

// (c): IN holds the ring value in every lane
#define STEP_C(SELB, SELN)                                                                            \
  asm volatile("v_max_i32 %[t0], %[a], %[x]\n\t"                                                      \
               "v_max3_i32 %[t], %[a], %[x], %[in]\n\t"                                               \
               "v_add_u32_sdwa %[b], %[x], sext(%[swb])" SDWA(SELB)                                   \
               "s_nop 0\n\t"                                                                          \
               "v_max_i32_dpp %[t], %[x2], %[t0]" DPPC                                                \
               "v_mov_b32_dpp %[in], %[x2]" DPPC                                                      \
               "v_add_u32_sdwa %[an], %[in], sext(%[swn])" SDWA(SELN)                                 \
               "v_max3_i32 %[h2], %[b], %[t], %[x2]"                                                  \
               : [t0] "=&v"(t0), [t] "=&v"(t), [b] "=&v"(b), [in] "+v"(in), [an] "=&v"(an), [h2] "=&v"(h2) \
               : [a] "v"(a), [x] "v"(X), [x2] "v"(X2), [swb] "v"(swb), [swn] "v"(swn))

template <int KK>
__device__ __forceinline__ void step_c(int& a, int& X, int& X2, int& in, unsigned swb, unsigned swn) {
  int t0, t, b, an, h2;
  if constexpr (KK == 0) STEP_C(0, 1);
  else if constexpr (KK == 1) STEP_C(1, 2);
  else if constexpr (KK == 2) STEP_C(2, 3);
  else STEP_C(3, 0);
  a = an;
  X = t;
  X2 = h2;
}

// (d): R = 1.  in: a = U + s; out: X = h, IN = the next diagonal, a = the next U + s
#define STEP_D(SELN)                                                                                  \
  asm volatile("v_max_i32 %[t], %[a], %[in]\n\t"                                                      \
               "s_nop 1\n\t"                                                                          \
               "v_max_i32_dpp %[t], %[x], %[t]" DPPC                                                  \
               "v_mov_b32_dpp %[in], %[x]" DPPC                                                       \
               "v_max_i32 %[h], %[t], %[x]\n\t"                                                       \
               "v_add_u32_sdwa %[an], %[in], sext(%[swn])" SDWA(SELN)                                 \
               : [t] "=&v"(t), [in] "+v"(in), [an] "=&v"(an), [h] "=&v"(h)                           \
               : [a] "v"(a), [x] "v"(X), [swn] "v"(swn))

template <int KK>
__device__ __forceinline__ void step_d(int& a, int& X, int& in, unsigned swn) {
  int t, an, h;
  if constexpr (KK == 0) STEP_D(1);
  else if constexpr (KK == 1) STEP_D(2);
  else if constexpr (KK == 2) STEP_D(3);
  else STEP_D(0);
  a = an;
  X = h;
}

template <int V>
__global__ void kstep(int* out, unsigned long long* cyc, int nphase) {
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  unsigned plo = 0x01000000u * lane + 0x00020001u, phi = 0x00010203u;
  unsigned plo2 = plo ^ 0x01010101u, phi2 = phi ^ 0x02020202u;
  asm("" : "+v"(plo), "+v"(phi), "+v"(plo2), "+v"(phi2));
  int X = lane, U = lane - 1, X2 = lane + 1;
  constexpr bool NEUTRAL = (V == 1 || V == 2 || V == 5 || V == 7);
  int inb = (NEUTRAL && lane != 0) ? NEG : 5;  // a phase's ring inputs: one v_mov each in every variant
  asm("" : "+v"(inb));
  int acc = 0, spare = lane;
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int q = 0; q < nphase; ++q) {
    int IN[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      IN[k] = inb;
      asm("" : "+v"(IN[k]));
    }
    unsigned cw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { cw[u] = (unsigned)(q * 0x01010101u + u + lane); asm("" : "+v"(cw[u])); }
    if constexpr (V == 0 || V == 4 || V == 6) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned s4 = __builtin_amdgcn_perm(phi, plo, cw[u]);
        const unsigned s4b = __builtin_amdgcn_perm(phi2, plo2, cw[u]);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int kx = 4 * u + kk;
          const int s = ((int)(s4 << (24 - 8 * kk))) >> 24;
          const int up = dpp_shr1(IN[kx], V != 4 ? X2 : X);
          int h1 = imax3(U + s, up, X);
          asm("" : "+v"(h1));
          U = up;
          const int xp = X;
          X = h1;
          if constexpr (V == 6) asm volatile("v_add_u32 %0, 1, %0" : "+v"(spare));
          if constexpr (V != 4) {
            const int sb = ((int)(s4b << (24 - 8 * kk))) >> 24;
            int h2 = imax3(xp + sb, X, X2);
            asm("" : "+v"(h2));
            X2 = h2;
          }
        }
      }
    } else if constexpr (V == 8) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned s4 = __builtin_amdgcn_perm(phi, plo, cw[u]);
        const unsigned s4b = __builtin_amdgcn_perm(phi2, plo2, cw[u]);
        step_a<0>(U, X, X2, IN[4 * u + 0], s4, s4b);
        step_a<1>(U, X, X2, IN[4 * u + 1], s4, s4b);
        step_a<2>(U, X, X2, IN[4 * u + 2], s4, s4b);
        step_a<3>(U, X, X2, IN[4 * u + 3], s4, s4b);
      }
    } else {
      unsigned s4 = __builtin_amdgcn_perm(phi, plo, cw[0]);
      unsigned s4b = __builtin_amdgcn_perm(phi2, plo2, cw[0]);
      int a = U + (((int)(s4 << 24)) >> 24);  // step 0's diagonal term
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        unsigned s4n = 0, s4bn = 0;
        if constexpr (V != 2) {
          s4n = __builtin_amdgcn_perm(phi, plo, cw[(u + 1) & 3]);
          s4bn = __builtin_amdgcn_perm(phi2, plo2, cw[(u + 1) & 3]);
        }
        const unsigned cwn = cw[(u + 1) & 3];
        if constexpr (V == 1) {
          step_b<0, 0>(a, X, X2, IN[4 * u + 0], s4b, s4, s4n, plo, phi, cwn);
          step_b<1, 0>(a, X, X2, IN[4 * u + 1], s4b, s4, s4n, plo, phi, cwn);
          step_b<2, 0>(a, X, X2, IN[4 * u + 2], s4b, s4, s4n, plo, phi, cwn);
          step_b<3, 0>(a, X, X2, IN[4 * u + 3], s4b, s4n, s4n, plo, phi, cwn);
        } else if constexpr (V == 2) {
          step_b<0, 1>(a, X, X2, IN[4 * u + 0], s4b, s4, s4n, plo, phi, cwn);
          step_b<1, 2>(a, X, X2, IN[4 * u + 1], s4b, s4, s4bn, plo2, phi2, cwn);
          step_b<2, 0>(a, X, X2, IN[4 * u + 2], s4b, s4, s4n, plo, phi, cwn);
          step_b<3, 0>(a, X, X2, IN[4 * u + 3], s4b, s4n, s4n, plo, phi, cwn);
        } else if constexpr (V == 7) {
          step_b2<0>(a, X, X2, IN[4 * u + 0], s4b, s4);
          step_b2<1>(a, X, X2, IN[4 * u + 1], s4b, s4);
          step_b2<2>(a, X, X2, IN[4 * u + 2], s4b, s4);
          step_b2<3>(a, X, X2, IN[4 * u + 3], s4b, s4n);
        } else if constexpr (V == 3) {
          step_c<0>(a, X, X2, IN[4 * u + 0], s4b, s4);
          step_c<1>(a, X, X2, IN[4 * u + 1], s4b, s4);
          step_c<2>(a, X, X2, IN[4 * u + 2], s4b, s4);
          step_c<3>(a, X, X2, IN[4 * u + 3], s4b, s4n);
        } else {
          step_d<0>(a, X, IN[4 * u + 0], s4);
          step_d<1>(a, X, IN[4 * u + 1], s4);
          step_d<2>(a, X, IN[4 * u + 2], s4);
          step_d<3>(a, X, IN[4 * u + 3], s4n);
        }
        s4 = s4n;
        s4b = s4bn;
      }
      U = IN[15];  // (the last block's a belongs to the next phase's codes: recomputed there)
      asm("" :: "v"(a));
    }
    acc ^= X + X2;
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (lane == 0) cyc[w] = t1 - t0;
  if (acc == 0x7fffffff) out[threadIdx.x] = acc + U + spare;
}

template <int V>
void run(const char* name, unsigned long long* d_cyc, int* d_out) {
  const int nphase = 4000;
  for (int waves : {1, 4}) {
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(kstep<V>, dim3(1), dim3(64 * waves), 0, 0, d_out, d_cyc, nphase);
    (void)hipDeviceSynchronize();
    unsigned long long c[4];
    (void)hipMemcpy(c, d_cyc, 8 * waves, hipMemcpyDeviceToHost);
    double t = 0;
    for (int w = 0; w < waves; ++w) t += (double)c[w] / (nphase * 16) / waves;
    std::printf("%-44s %d wave%s: %6.2f ticks/step\n", name, waves, waves > 1 ? "s" : " ", t);
  }
}

int main() {
  unsigned long long* d_cyc;
  int* d_out;
  (void)hipMalloc(&d_cyc, 64);
  (void)hipMalloc(&d_out, 4096);
  run<0>("(a)  R=2 DPP -> max3 -> max3 (today)", d_cyc, d_out);
  run<8>("(a*) today's step, hand-ordered a, b, DPP, h1, h2", d_cyc, d_out);
  run<1>("(b)  R=2 fused, neutral input, s_nop filler", d_cyc, d_out);
  run<2>("(b') R=2 fused, neutral input, perm fillers", d_cyc, d_out);
  run<7>("(b2) R=2 fused, neutral input, no filler", d_cyc, d_out);
  run<3>("(c)  R=2 fused, extra v_max", d_cyc, d_out);
  run<4>("     R=1 DPP -> max3 (today)", d_cyc, d_out);
  run<5>("(d)  R=1 fused", d_cyc, d_out);
  run<6>("(a+) (a) and one independent VALU per step", d_cyc, d_out);
  return 0;
}
