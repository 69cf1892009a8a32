// Issue cost of k_fill8's pair of rows with gaps opened from the diagonal candidate only (xc = x - (gapO - gapE) for two rows in one
// v_lshl_add_u64, off the serial chain) against today's pair of rows (t = h - (gapO - gapE), one v_sub_u32 per row inside the chain):
//   today   1 pair add + 2 x (max3, sub, max3, pk_max)      9 instructions per pair of rows
//   diag    2 pair ops + 2 x (max3, max3, max3)             8 instructions per pair of rows (F's maximum takes the floor as E's does)
//   hipcc --offload-arch=gfx950 -O3 -o diaggap_issue_probe diaggap_issue_probe.hip && ./diaggap_issue_probe
// One wavefront per SIMD and block, `occ` blocks per CU (held there by the LDS request); five timed repeats per cell, minimum and
// maximum given.  The shader clock is measured per launch: cycle counter against the constant-rate wall clock inside the kernel.
// The kernels keep their operands in fixed registers v[16:37] (clobbered): a 64-bit asm operand has no name for its halves.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
typedef uint32_t u32;
typedef unsigned long long u64;

#define R2(x) x x
#define R4(x) R2(x) R2(x)
#define CLOB "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", \
             "v32", "v33", "v34", "v35", "v36", "v37"

// v[16:17] v[18:19]: pair sums x; v[20:21] v[22:23]: H pairs; v[24:25]: profile pair; v26 v27: E of the two rows; v28: f; v29: h; v30: t;
// v31: c1 / floor; v[32:33] v[34:35]: xc pairs; v[36:37]: -(c1:c1) as one 64-bit addend
#define PADD(d, a) "v_lshl_add_u64 v[" #d "], v[" #a "], 0, v[24:25]\n\t"
#define PSUB(d, a) "v_lshl_add_u64 v[" #d "], v[" #a "], 0, v[36:37]\n\t"
#define MAX3(d, a, b, c) "v_pk_maximum3_f16 v" #d ", v" #a ", v" #b ", v" #c "\n\t"
#define SUB(d, a, b) "v_sub_u32 v" #d ", v" #a ", v" #b "\n\t"
#define PKMAX(d, a, b) "v_pk_max_i16 v" #d ", v" #a ", v" #b "\n\t"
// today's row without its diagonal add: h = max3(x, E, f); t = h - c1; E = max3(E, t, floor); f = max(f, t)
#define ROW(x, e) MAX3(29, x, e, 28) SUB(30, 29, 31) MAX3(e, e, 30, 31) PKMAX(28, 28, 30)
// the row with gaps from the diagonal: h = max3(x, E, f); E = max3(xc, E, floor); f = max3(xc, f, floor)
#define ROWD(x, xc, e) MAX3(29, x, e, 28) MAX3(e, xc, e, 31) MAX3(28, xc, 28, 31)

// two pairs of rows per pass, each pair add formed one pair ahead of its rows (it reads the H pair, not the chain)
#define BODY_today R2(PADD(16:17, 20:21) ROW(18, 26) ROW(19, 27) PADD(18:19, 22:23) ROW(16, 26) ROW(17, 27))
#define BODY_diag R2(PADD(16:17, 20:21) PSUB(32:33, 16:17) ROWD(18, 34, 26) ROWD(19, 35, 27) \
                     PADD(18:19, 22:23) PSUB(34:35, 18:19) ROWD(16, 32, 26) ROWD(17, 33, 27))
// the same with the pair subtract as two 32-bit subtracts (what the 64-bit form has to beat)
#define BODY_diag32 R2(PADD(16:17, 20:21) SUB(32, 16, 31) SUB(33, 17, 31) ROWD(18, 34, 26) ROWD(19, 35, 27) \
                       PADD(18:19, 22:23) SUB(34, 18, 31) SUB(35, 19, 31) ROWD(16, 32, 26) ROWD(17, 33, 27))

#define KERNEL(NAME) \
__global__ void __launch_bounds__(256) k_##NAME(u32* sink, u64* clk, int iters, u32 g) { \
  extern __shared__ u32 lds[]; const u32 gid = blockIdx.x * 256 + threadIdx.x; \
  const u64 c0 = clock64(), w0 = wall_clock64(); \
  asm volatile("v_mov_b32 v16, %0\n\tv_mov_b32 v17, %0\n\tv_mov_b32 v18, %0\n\tv_mov_b32 v19, %0\n\tv_mov_b32 v20, %0\n\tv_mov_b32 v21, %0\n\t" \
               "v_mov_b32 v22, %0\n\tv_mov_b32 v23, %0\n\tv_mov_b32 v24, %1\n\tv_mov_b32 v25, %1\n\tv_mov_b32 v26, %0\n\tv_mov_b32 v27, %0\n\t" \
               "v_mov_b32 v28, %0\n\tv_mov_b32 v29, %0\n\tv_mov_b32 v30, %0\n\tv_mov_b32 v31, %1\n\tv_mov_b32 v32, %0\n\tv_mov_b32 v33, %0\n\t" \
               "v_mov_b32 v34, %0\n\tv_mov_b32 v35, %0\n\tv_sub_u32 v36, 0, %1\n\tv_not_b32 v37, %1" : : "v"(gid), "v"(g) : CLOB); \
  for (int it = 0; it < iters; ++it) asm volatile(BODY_##NAME : : : CLOB); \
  u32 out; asm volatile("v_xor_b32 %0, v16, v18\n\tv_xor_b32 %0, %0, v26\n\tv_xor_b32 %0, %0, v28" : "=v"(out) : : CLOB); \
  const u64 c1 = clock64(), w1 = wall_clock64(); \
  if (iters < 0) lds[threadIdx.x] = out; \
  sink[gid] = out; \
  if (gid == 0) { clk[0] = c1 - c0; clk[1] = w1 - w0; } }

KERNEL(today) KERNEL(diag) KERNEL(diag32)

static double wall_hz;

// ninstr: vector instructions per loop trip; npairs: pairs of rows per trip
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
    printf("  occ%d %5.2f..%5.2f (%6.2f..%6.2f /pair)", occ, lo, hi, lo * ninstr / npairs, hi * ninstr / npairs);
    if (occ == 8) printf("  %4.0f MHz", mhz);
  }
  printf("\n");
}

int main()
{
  u32* sink; u64* clk;
  if (hipMalloc(&sink, 256 * 32 * 4 * 256 * 4) != hipSuccess || hipMalloc(&clk, 16) != hipSuccess) { printf("no device memory\n"); return 1; }
  int khz = 0; hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0); wall_hz = khz * 1e3;
  printf("SIMD cycles per vector instruction and per pair of rows (minimum..maximum of five repeats); clock as measured\n");
  run("today", k_today, 36, 4, sink, clk);
  run("diag", k_diag, 32, 4, sink, clk);
  run("diag32", k_diag32, 40, 4, sink, clk);
  run("today", k_today, 36, 4, sink, clk);
  run("diag", k_diag, 32, 4, sink, clk);
  return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
