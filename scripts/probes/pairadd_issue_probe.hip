// Issue cost of v_lshl_add_u64 (one 64-bit add forming diag + score of two neighbouring rows of k_fill8) on gfx950:
// alone, alternating with v_pk_maximum3_f16, and in a row-shaped mix against the same mix with two v_add_u32 in its place.
//   hipcc --offload-arch=gfx950 -O3 -o pairadd_issue_probe pairadd_issue_probe.hip && ./pairadd_issue_probe
// One wavefront per SIMD and block, `occ` blocks per CU (held there by the LDS request); five timed repeats per cell, minimum and
// maximum given.  The shader clock is measured per launch: cycle counter against the constant-rate wall clock inside the kernel.
// The kernels keep their operands in fixed registers v[16:31] (clobbered): a 64-bit asm operand has no name for its halves.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
typedef uint32_t u32;
typedef unsigned long long u64;

#define R2(x) x x
#define R4(x) R2(x) R2(x)
#define R8(x) R4(x) R4(x)
#define R16(x) R8(x) R8(x)
#define CLOB "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31"

// v[16:17] v[18:19] v[20:21] v[22:23]: pair sums / H pairs; v[24:25]: profile pair; v26 v27: E of the two rows; v28: f; v29: h; v30: t; v31: c1 / floor
#define PADD(d, a) "v_lshl_add_u64 v[" #d "], v[" #a "], 0, v[24:25]\n\t"
#define MAX3(d, a, b, c) "v_pk_maximum3_f16 v" #d ", v" #a ", v" #b ", v" #c "\n\t"
#define ADD(d, a, b) "v_add_u32 v" #d ", v" #a ", v" #b "\n\t"
#define SUB(d, a, b) "v_sub_u32 v" #d ", v" #a ", v" #b "\n\t"
#define PKMAX(d, a, b) "v_pk_max_i16 v" #d ", v" #a ", v" #b "\n\t"
// one row of chain_row8 without its diagonal add: h = max3(x, E, f); t = h - c1; E = max3(E, t, floor); f = max(f, t)
#define ROW(x, e) MAX3(29, x, e, 28) SUB(30, 29, 31) MAX3(e, e, 30, 31) PKMAX(28, 28, 30)

// 4 independent pair adds
#define BODY_P_only R4(PADD(16:17, 16:17) PADD(18:19, 18:19) PADD(20:21, 20:21) PADD(22:23, 22:23))
// 4 independent 32-bit adds (reference)
#define BODY_A_only R4(ADD(16, 16, 24) ADD(18, 18, 24) ADD(20, 20, 24) ADD(22, 22, 24))
// 4 independent max3 (reference)
#define BODY_X_only R4(MAX3(26, 26, 24, 25) MAX3(27, 27, 24, 25) MAX3(28, 28, 24, 25) MAX3(29, 29, 24, 25))
// pair add alternating with max3, as the compiler places them
#define BODY_P1X1 R4(PADD(16:17, 16:17) MAX3(26, 26, 24, 25) PADD(18:19, 18:19) MAX3(27, 27, 24, 25))
#define BODY_A1X1 R4(ADD(16, 16, 24) MAX3(26, 26, 24, 25) ADD(18, 18, 24) MAX3(27, 27, 24, 25))
// two rows: the pair add (of the NEXT pair: independent of the chain, reads the H pair) and the rows' serial chain
#define BODY_rowP R2(PADD(16:17, 20:21) ROW(18, 26) ROW(19, 27) PADD(18:19, 22:23) ROW(16, 26) ROW(17, 27))
#define BODY_rowA R2(ADD(16, 20, 24) ADD(17, 21, 25) ROW(18, 26) ROW(19, 27) ADD(18, 22, 24) ADD(19, 23, 25) ROW(16, 26) ROW(17, 27))

#define KERNEL(NAME) \
__global__ void __launch_bounds__(256) k_##NAME(u32* sink, u64* clk, int iters, u32 g) { \
  extern __shared__ u32 lds[]; const u32 gid = blockIdx.x * 256 + threadIdx.x; \
  const u64 c0 = clock64(), w0 = wall_clock64(); \
  asm volatile("v_mov_b32 v16, %0\n\tv_mov_b32 v17, %0\n\tv_mov_b32 v18, %0\n\tv_mov_b32 v19, %0\n\tv_mov_b32 v20, %0\n\tv_mov_b32 v21, %0\n\t" \
               "v_mov_b32 v22, %0\n\tv_mov_b32 v23, %0\n\tv_mov_b32 v24, %1\n\tv_mov_b32 v25, %1\n\tv_mov_b32 v26, %0\n\tv_mov_b32 v27, %0\n\t" \
               "v_mov_b32 v28, %0\n\tv_mov_b32 v29, %0\n\tv_mov_b32 v30, %0\n\tv_mov_b32 v31, %1" : : "v"(gid), "v"(g) : CLOB); \
  for (int it = 0; it < iters; ++it) asm volatile(BODY_##NAME : : : CLOB); \
  u32 out; asm volatile("v_xor_b32 %0, v16, v18\n\tv_xor_b32 %0, %0, v26\n\tv_xor_b32 %0, %0, v28" : "=v"(out) : : CLOB); \
  const u64 c1 = clock64(), w1 = wall_clock64(); \
  if (iters < 0) lds[threadIdx.x] = out; \
  sink[gid] = out; \
  if (gid == 0) { clk[0] = c1 - c0; clk[1] = w1 - w0; } }

KERNEL(P_only) KERNEL(A_only) KERNEL(X_only) KERNEL(P1X1) KERNEL(A1X1) KERNEL(rowP) KERNEL(rowA)

static double wall_hz;

// ninstr: vector instructions per loop trip; npairs: pairs of rows per trip (0: not a row mix)
template <typename K> void run(const char* name, K kern, int ninstr, int npairs, u32* sink, u64* clk)
{
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  printf("%-8s", name);
  for (int occ = 1; occ <= 8; occ *= 2) {
    size_t lds = occ >= 8 ? 0 : (160 * 1024) / occ - 1024;
    hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const int blocks = 256 * occ * 4, iters = 4000;
    kern<<<blocks, 256, lds>>>(sink, clk, 10, 3u); hipDeviceSynchronize();
    double lo = 1e30, hi = 0, mhz = 0;
    for (int r = 0; r < 5; ++r) {
      hipEventRecord(a); kern<<<blocks, 256, lds>>>(sink, clk, iters, 3u); hipEventRecord(b); hipEventSynchronize(b);
      float ms; hipEventElapsedTime(&ms, a, b);
      u64 c[2]; hipMemcpy(c, clk, sizeof c, hipMemcpyDeviceToHost);
      double hz = c[1] ? (double)c[0] / (double)c[1] * wall_hz : 0;
      if (hz < 5e8 || hz > 4e9) hz = 2.4e9;      // a cycle counter that does not run at the shader clock: nominal clock instead
      mhz += hz * 1e-6 / 5;
      // one wavefront per SIMD and block: wavefront instructions per SIMD = blocks / 256 * iters * ninstr
      const double cyc = ms * 1e-3 * hz / ((double)blocks / 256.0 * iters * ninstr);
      if (cyc < lo) lo = cyc;
      if (cyc > hi) hi = cyc;
    }
    printf("  occ%d %5.2f..%5.2f", occ, lo, hi);
    if (npairs) printf(" (%6.2f..%6.2f /pair)", lo * ninstr / npairs, hi * ninstr / npairs);
    if (occ == 8) printf("  %4.0f MHz", mhz);
  }
  printf("\n");
}

int main()
{
  u32* sink; u64* clk; hipMalloc(&sink, 256 * 32 * 4 * 256 * 4); hipMalloc(&clk, 16);
  int khz = 0; hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0); wall_hz = khz * 1e3;
  printf("SIMD cycles per vector instruction (minimum..maximum of five repeats), per pair of rows for the row mixes; clock as measured\n");
  run("P_only", k_P_only, 16, 0, sink, clk);
  run("A_only", k_A_only, 16, 0, sink, clk);
  run("X_only", k_X_only, 16, 0, sink, clk);
  run("P1X1", k_P1X1, 16, 0, sink, clk);
  run("A1X1", k_A1X1, 16, 0, sink, clk);
  run("rowP", k_rowP, 36, 4, sink, clk);
  run("rowA", k_rowA, 40, 4, sink, clk);
  return 0;
}
