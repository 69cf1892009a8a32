// Issue cost of ONE STEP of k_fill8<19, dg> as it stands against three ways of taking vector instructions out of it:
//   a   as today: nine pairs of rows (2 pair ops + 2 x 3 maxima of three), the odd row with its own add and subtract, the 13-instruction
//       class reduction, four serial v_sub_u32 on the F chain, three DPP hand-offs, floor add, address add           99 vector instructions
//   b   the plain adds in pairs: (a1 : a2) - (g : 2g), and each of F's four subtracts in one v_lshl_add_u64 with an independent add --
//       the floor, the next step's profile address, x of the odd row, a3 - 3g                                         94
//   c   b, and the column maximum goes down through LDS (one ds_write_b32 + one ds_read_b32 for the v_mov_b32_dpp)      93
//   d   c, and H goes down through LDS too (the two head lanes store their floor under an execution mask)             92
// every variant with five ds_read_b128 of profile words and one ds_read_u16 of the target ring per step, read a step ahead.
//   hipcc --offload-arch=gfx950 -O3 -o handoff_issue_probe handoff_issue_probe.hip && ./handoff_issue_probe
// One wavefront per SIMD and block, `occ` blocks per CU (held there by the LDS request); five timed repeats per cell, minimum and
// maximum given.  The shader clock is measured per launch: cycle counter against the constant-rate wall clock inside the kernel.
// The kernels keep their operands in fixed registers v[16:99] (clobbered): a 64-bit asm operand has no name for its halves.
// LDS: 8 KiB static per block.  0 .. 5119 profile words (lane x 16 B + 1 KiB x quad), 5120 the ring entry (zero, never written in the
// loop, so every profile address stays lane x 16), 6144 .. 8191 the hand-off slots (512 B per wavefront: 64 x 4 B per handed value; a lane
// reads slot (lane - 2) mod 64 of its own wavefront).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
typedef uint32_t u32;
typedef unsigned long long u64;

#define CLOB "memory", "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", \
             "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", \
             "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", \
             "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", \
             "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", \
             "v96", "v97", "v98", "v99"

// v[16:17] v[18:19]: pair sums x; v[20:21] v[22:23]: H pairs; v26 v27: E of the two rows; v29: h; v31: c1; v[32:33] v[34:35]: xc pairs;
// v[36:37]: -(c1:c1); v[40:59]: the five profile quads; v60: lane x 16; v63 / v64: own / left neighbour's hand-off slot; v65: ring slot;
// v66: hin; v67: column maximum from above; v70: 4g; v71: g; v72 v74 v75 v94: a0 a1 a2 a3; v80: floor; v84: ring entry / profile address;
// v86 .. v89, v96 .. v99: the addends of the pairs; v90: H of row 17; f: v28 -> v81 -> v85 -> v91 -> v93 -> v95
#define PADD(d, a, s) "v_lshl_add_u64 v[" #d "], v[" #a "], 0, v[" #s "]\n\t"
#define PSUB(d, a) "v_lshl_add_u64 v[" #d "], v[" #a "], 0, v[36:37]\n\t"
#define MAX3(d, a, b, c) "v_pk_maximum3_f16 v" #d ", v" #a ", v" #b ", v" #c "\n\t"
#define ADD(d, a, b) "v_add_u32 v" #d ", v" #a ", v" #b "\n\t"
#define SUB(d, a, b) "v_sub_u32 v" #d ", v" #a ", v" #b "\n\t"
#define PKMAX(d, a, b) "v_pk_max_i16 v" #d ", v" #a ", v" #b "\n\t"
#define WAIT(n) "s_waitcnt lgkmcnt(" #n ")\n\t"
// the row with gaps from the diagonal: h = max3(x, E, f); E = max3(xc, E, floor); f' = max3(xc, f, floor)
#define ROWD(x, xc, e, fi, fo) MAX3(29, x, e, fi) MAX3(e, xc, e, 80) MAX3(fo, xc, fi, 80)
// a pair of rows and the pair ops that form the NEXT pair's x and xc (they read the H pair, not the chain); A / B alternate the registers
#define UNIT_A(s, f0, f1) PADD(16:17, 20:21, s) PSUB(32:33, 16:17) ROWD(18, 34, 26, f0, f1) ROWD(19, 35, 27, f1, f1)
#define UNIT_B(s, f0, f1) PADD(18:19, 22:23, s) PSUB(34:35, 18:19) ROWD(16, 32, 26, f0, f1) ROWD(17, 33, 27, f1, f1)
// the step's profile words, then the ring entry of the step after (in-order LDS queue: lgkmcnt(5 - k) means quad k has landed)
#define LOADS "ds_read_b128 v[40:43], v84\n\tds_read_b128 v[44:47], v84 offset:1024\n\tds_read_b128 v[48:51], v84 offset:2048\n\t" \
              "ds_read_b128 v[52:55], v84 offset:3072\n\tds_read_b128 v[56:59], v84 offset:4096\n\tds_read_u16 v84, v65\n\t"
#define DPP_H "s_nop 4\n\tv_max_u32_dpp v66, v21, v80 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
#define DPP_F "s_nop 4\n\tv_sub_u32_dpp v28, v95, v71 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
#define DPP_CM "s_nop 1\n\tv_mov_b32_dpp v72, v67 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"

// a: every plain add on its own.  Accumulator maxima as chain_row8 places them at R8 = 19 (class 0 starts from the maximum handed in)
#define STEP_a DPP_H DPP_F DPP_CM LOADS WAIT(5) \
  UNIT_A(40:41, 28, 81) UNIT_B(42:43, 81, 81) SUB(81, 81, 70) ADD(80, 80, 86) WAIT(4) MAX3(75, 75, 20, 29) \
  UNIT_A(44:45, 81, 85) MAX3(72, 72, 20, 29) UNIT_B(46:47, 85, 85) SUB(85, 85, 70) WAIT(0) ADD(84, 84, 88) MAX3(94, 94, 20, 29) \
  UNIT_A(48:49, 85, 91) MAX3(74, 74, 20, 29) UNIT_B(50:51, 91, 91) SUB(91, 91, 70) MAX3(75, 75, 20, 29) \
  UNIT_A(52:53, 91, 95) MAX3(72, 72, 20, 29) UNIT_B(54:55, 95, 95) PKMAX(94, 94, 29) SUB(95, 95, 70) \
  UNIT_A(56:57, 95, 95) MAX3(74, 74, 20, 29) ADD(92, 90, 58) SUB(32, 92, 31) ROWD(92, 32, 26, 95, 95) MAX3(75, 75, 20, 29) \
  SUB(76, 74, 71) SUB(77, 75, 71) SUB(94, 94, 71) MAX3(67, 72, 20, 76) MAX3(67, 67, 77, 94)
// b: (fl : f) + (g : -4g) after row 3, (address : f) + (lane : -4g) after row 7, (H17 : f) + (s18 : -4g) after row 11 with the addend out of
// the profile quad, (a3 : f) - (3g : 4g) after row 15, (a1 : a2) - (g : 2g) in the reduction; xc of the odd row stays alone
#define ROWS_b \
  UNIT_A(40:41, 28, 81) UNIT_B(42:43, 81, 81) PADD(80:81, 80:81, 86:87) WAIT(4) MAX3(75, 75, 20, 29) \
  UNIT_A(44:45, 81, 85) MAX3(72, 72, 20, 29) UNIT_B(46:47, 85, 85) WAIT(0) PADD(84:85, 84:85, 88:89) MAX3(94, 94, 20, 29) \
  UNIT_A(48:49, 85, 91) MAX3(74, 74, 20, 29) UNIT_B(50:51, 91, 91) PADD(92:93, 90:91, 58:59) MAX3(75, 75, 20, 29) \
  UNIT_A(52:53, 93, 95) MAX3(72, 72, 20, 29) UNIT_B(54:55, 95, 95) PKMAX(94, 94, 29) PADD(94:95, 94:95, 96:97) \
  UNIT_A(56:57, 95, 95) MAX3(74, 74, 20, 29) SUB(32, 92, 31) ROWD(92, 32, 26, 95, 95) MAX3(75, 75, 20, 29) \
  PADD(76:77, 74:75, 98:99)
#define STEP_b DPP_H DPP_F DPP_CM LOADS WAIT(5) ROWS_b MAX3(67, 72, 20, 76) MAX3(67, 67, 77, 94)
// c: the column maximum through LDS -- stored at the end of a step, loaded at once, folded in at the END of class 0 of the next step
#define CM_LDS "ds_write_b32 v63, v67\n\tds_read_b32 v68, v64\n\t"
#define STEP_c DPP_H DPP_F LOADS WAIT(5) ROWS_b MAX3(67, 72, 68, 76) MAX3(67, 67, 77, 94) CM_LDS
// d: H through LDS too; the two head lanes of every row store the floor into their own slots under an execution mask
#define H_LDS "ds_write_b32 v63, v21 offset:256\n\ts_mov_b64 exec, %0\n\tds_write_b32 v63, v80 offset:256\n\ts_mov_b64 exec, -1\n\t" \
              "ds_read_b32 v66, v64 offset:256\n\t"
#define STEP_d DPP_F LOADS WAIT(5) ROWS_b MAX3(67, 72, 68, 76) MAX3(67, 67, 77, 94) CM_LDS H_LDS

#define KERNEL(NAME) \
__global__ void __launch_bounds__(256) k_##NAME(u32* sink, u64* clk, int iters, u32 g) { \
  __shared__ __attribute__((aligned(16))) u32 slds[2048]; \
  extern __shared__ u32 lds[]; const u32 tid = threadIdx.x, gid = blockIdx.x * 256 + tid; \
  for (u32 i = tid; i < 2048; i += 256) slds[i] = i < 1280 ? (g + (i & 3)) * 0x10001u : 0u; \
  __syncthreads(); \
  const u32 base = (u32)(uintptr_t)(__attribute__((address_space(3))) u32*)slds, lane = tid & 63, own = base + 6144 + (tid >> 6) * 512 + lane * 4, \
            left = base + 6144 + (tid >> 6) * 512 + ((lane - 2) & 63) * 4, prof = base + lane * 16, ringslot = base + 5120; \
  const u64 heads = 0x0003000300030003ull; \
  const u64 c0 = clock64(), w0 = wall_clock64(); \
  asm volatile("v_mov_b32 v16, %0\n\tv_mov_b32 v17, %0\n\tv_mov_b32 v18, %0\n\tv_mov_b32 v19, %0\n\tv_mov_b32 v20, %0\n\tv_mov_b32 v21, %0\n\t" \
               "v_mov_b32 v22, %0\n\tv_mov_b32 v23, %0\n\tv_mov_b32 v26, %0\n\tv_mov_b32 v27, %0\n\tv_mov_b32 v28, %0\n\tv_mov_b32 v29, %0\n\t" \
               "v_mov_b32 v31, %1\n\tv_mov_b32 v32, %0\n\tv_mov_b32 v33, %0\n\tv_mov_b32 v34, %0\n\tv_mov_b32 v35, %0\n\t" \
               "v_sub_u32 v36, 0, %1\n\tv_not_b32 v37, %1\n\tv_mov_b32 v66, %0\n\tv_mov_b32 v67, %0\n\tv_mov_b32 v68, %0\n\t" \
               "v_lshlrev_b32 v70, 2, %1\n\tv_mov_b32 v71, %1\n\tv_mov_b32 v72, %0\n\tv_mov_b32 v74, %0\n\tv_mov_b32 v75, %0\n\t" \
               "v_mov_b32 v76, %0\n\tv_mov_b32 v77, %0\n\tv_mov_b32 v80, %0\n\tv_mov_b32 v81, %0\n\tv_mov_b32 v85, %0\n\t" \
               "v_mov_b32 v86, %1\n\tv_sub_u32 v87, 0, v70\n\tv_mov_b32 v89, v87\n\tv_mov_b32 v90, %0\n\tv_mov_b32 v91, %0\n\t" \
               "v_mov_b32 v92, %0\n\tv_mov_b32 v93, %0\n\tv_mov_b32 v94, %0\n\tv_mov_b32 v95, %0\n\tv_mul_u32_u24 v96, -3, %1\n\tv_not_b32 v97, v70\n\t" \
               "v_sub_u32 v98, 0, %1\n\tv_not_b32 v99, %1\n\t" \
               "v_mov_b32 v60, %2\n\tv_mov_b32 v84, %2\n\tv_mov_b32 v88, %2\n\tv_mov_b32 v63, %3\n\tv_mov_b32 v64, %4\n\tv_mov_b32 v65, %5" \
               : : "v"(gid & 0xfffu), "v"(g), "v"(prof), "v"(own), "v"(left), "v"(ringslot) : CLOB); \
  /* (v88: the lane's share of the profile address; the ring entry it is added to is the zero at byte 5120) */ \
  for (int it = 0; it < iters; ++it) asm volatile(STEP_##NAME STEP_##NAME : : "s"(heads) : CLOB); \
  u32 out; asm volatile("s_waitcnt lgkmcnt(0)\n\tv_xor_b32 %0, v16, v18\n\tv_xor_b32 %0, %0, v26\n\tv_xor_b32 %0, %0, v95\n\tv_xor_b32 %0, %0, v67\n\tv_xor_b32 %0, %0, v66" : "=v"(out) : : CLOB); \
  const u64 c1 = clock64(), w1 = wall_clock64(); \
  if (iters < 0) lds[tid] = out; \
  sink[gid] = out; \
  if (gid == 0) { clk[0] = c1 - c0; clk[1] = w1 - w0; } }

KERNEL(a) KERNEL(b) KERNEL(c) KERNEL(d)

static double wall_hz;

// ninstr: vector instructions per step (two steps per loop trip)
template <typename K> void run(const char* name, K kern, int ninstr, u32* sink, u64* clk)
{
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  printf("%-3s %3d", name, ninstr);
  for (int occ = 1; occ <= 8; occ *= 2) {
    size_t lds = occ >= 8 ? 0 : (160 * 1024) / occ - 1024 - 8192;
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
      // one wavefront per SIMD and block: steps per SIMD = blocks / 256 * iters * 2
      const double cyc = ms * 1e-3 * hz / ((double)blocks / 256.0 * iters * 2);
      if (cyc < lo) lo = cyc;
      if (cyc > hi) hi = cyc;
    }
    printf("  occ%d %6.1f..%6.1f (%4.2f /instr)", occ, lo, hi, lo / ninstr);
    if (occ == 8) printf("  %4.0f MHz", mhz);
  }
  printf("\n");
}

int main()
{
  u32* sink; u64* clk;
  if (hipMalloc(&sink, 256 * 32 * 4 * 256 * 4) != hipSuccess || hipMalloc(&clk, 16) != hipSuccess) { printf("no device memory\n"); return 1; }
  int khz = 0; hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0); wall_hz = khz * 1e3;
  printf("SIMD cycles per step of the wavefront and SIMD (minimum..maximum of five repeats; per vector instruction at the minimum); clock as measured\n");
  for (int pass = 0; pass < 2; ++pass) {
    run("a", k_a, 99, sink, clk);
    run("b", k_b, 94, sink, clk);
    run("c", k_c, 93, sink, clk);
    run("d", k_d, 92, sink, clk);
  }
  return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
