// tools/lab/issue_lab.hip — what a gfx950 CU issues per cycle, by instruction class (lab code: not linked into libhipblosc.so).
//
// DESIGN.md §5.2 / §5.7 / §8 argue from an issue model (how many vector and how many scalar wave-instructions a CU takes per cycle).
// This program measures it for the instruction classes the LZ4 kernels are made of.  Single-wave workgroups, W = 1, 2, 4, 6 of them per
// SIMD on every CU (dynamic LDS sized so that exactly 4 W fit a CU); every wave runs a long unrolled stream of independent instructions
// of ONE class -- ALU and branch instructions only, nothing that touches memory -- and stamps the shader clock and the 100 MHz
// real-time clock around the stream (compiler builtins, outside the stream).  Results leave through ordinary C++ stores.  A launch is
// timed with HIP events.
//
//   rate    = wave-instructions / ns / CU, from the events (all waves of the launch)
//   cyc     = shader cycles per wave-instruction of ONE wave (median over waves, from its own stamps)
//   clk_ghz = shader clock while the stream ran (stamps: cycles per 10 ns tick)
//
// Mixes: `v+s one wave` alternates a vector and a scalar instruction in one stream; `v+s two waves` gives the waves of a SIMD the two
// streams by the parity of their hardware wave slot.
//
// The LDS sizing caps the waves of a CU at 4 W; it does not place them: the rates read as "W per SIMD" assume the dispatcher spread them evenly over
// the four SIMDs, and `waves_by_simd` in the output records the split each launch had (even at W = 1, 2, 4 where this was run).  Where a launch takes
// longer than its waves' own stamps account for, fewer than 4 W were resident at a time (W = 6 ran as two rounds of 16 workgroups per CU).
//
//   issue_lab [out.json] [iters]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(2); } } while (0)

struct Stamp { uint64_t c0, c1, r0, r1; uint32_t hwid, role, pad0, pad1; };

#define R8(I) I(0) I(1) I(2) I(3) I(4) I(5) I(6) I(7)
#define R4(I) I(0) I(1) I(2) I(3)
#define R128(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I)
#define S128(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) \
                R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I) R4(I)
constexpr int PER_ITER = 128;                     // instructions of the class per loop iteration (the loop adds s_add / s_cmp / s_cbranch)

__device__ __forceinline__ uint32_t hw_id() { return __builtin_amdgcn_s_getreg(4 | (31 << 11)); }      // HW_REG_HW_ID: wave slot [3:0], SIMD [5:4]
#define BEGIN() const uint64_t r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_amdgcn_s_memtime()
#define END(ROLE, SINK) do { const uint64_t c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();                       \
        if (threadIdx.x == 0) { Stamp s; s.c0 = c0; s.c1 = c1; s.r0 = r0; s.r1 = r1; s.hwid = hw_id(); s.role = (ROLE); s.pad0 = s.pad1 = 0; \
                                st[blockIdx.x] = s; }                                                                                          \
        sink[blockIdx.x * 64u + threadIdx.x] = (SINK); } while (0)

// ---- vector classes: 8 independent 32-bit accumulators %0..%7, two vector inputs %8 %9 ----
#define V_KERNEL(NAME, I, ...)                                                                                                   \
    __global__ __launch_bounds__(64) void NAME(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {                   \
        uint32_t v0 = threadIdx.x, v1 = v0 + 1, v2 = v0 + 2, v3 = v0 + 3, v4 = v0 + 4, v5 = v0 + 5, v6 = v0 + 6, v7 = v0 + 7;    \
        const uint32_t va = a + threadIdx.x, vb = b ^ threadIdx.x;                                                               \
        BEGIN();                                                                                                                 \
        for (int it = 0; it < iters; it++)                                                                                       \
            asm volatile(R128(I) : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7)                \
                         : "v"(va), "v"(vb) : __VA_ARGS__);                                                                      \
        END(0u, v0 ^ v1 ^ v2 ^ v3 ^ v4 ^ v5 ^ v6 ^ v7);                                                                          \
    }
#define I_AND(k)   "v_and_b32 %" #k ", %8, %" #k "\n"
#define I_PERM(k)  "v_perm_b32 %" #k ", %" #k ", %8, %9\n"
#define I_ALIGN(k) "v_alignbyte_b32 %" #k ", %" #k ", %8, %9\n"
#define I_MAD24(k) "v_mad_u32_u24 %" #k ", %" #k ", %8, %9\n"
#define I_CNDM(k)  "v_cndmask_b32_e32 %" #k ", %" #k ", %8, vcc\n"
#define I_FFBL(k)  "v_ffbl_b32_e32 %" #k ", %" #k "\n"
#define I_CMPVCC(k) "v_cmp_eq_u32_e32 vcc, %" #k ", %8\n"
V_KERNEL(k_v_and, I_AND, "memory")
V_KERNEL(k_v_perm, I_PERM, "memory")
V_KERNEL(k_v_alignbyte, I_ALIGN, "memory")
V_KERNEL(k_v_mad_u32_u24, I_MAD24, "memory")
V_KERNEL(k_v_cndmask, I_CNDM, "memory")
V_KERNEL(k_v_ffbl, I_FFBL, "memory")
V_KERNEL(k_v_cmp_vcc, I_CMPVCC, "vcc", "memory")
// the same select with its mask in a scalar register pair (VOP3), and a vector instruction with a scalar source: 8 accumulators %0..%7, vector
// input %8, a 64-bit and a 32-bit scalar input %9 %10
#define I_CNDM_SG(k) "v_cndmask_b32_e64 %" #k ", %" #k ", %8, %9\n"
#define I_AND_SG(k)  "v_and_b32 %" #k ", %10, %" #k "\n"
#define VS_KERNEL(NAME, I)                                                                                                       \
    __global__ __launch_bounds__(64) void NAME(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {                   \
        uint32_t v0 = threadIdx.x, v1 = v0 + 1, v2 = v0 + 2, v3 = v0 + 3, v4 = v0 + 4, v5 = v0 + 5, v6 = v0 + 6, v7 = v0 + 7;    \
        const uint32_t va = a + threadIdx.x; const uint64_t sm = ((uint64_t)b << 32) | a;                                        \
        BEGIN();                                                                                                                 \
        for (int it = 0; it < iters; it++)                                                                                       \
            asm volatile(R128(I) : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7)                \
                         : "v"(va), "s"(sm), "s"(b) : "memory");                                                                 \
        END(0u, v0 ^ v1 ^ v2 ^ v3 ^ v4 ^ v5 ^ v6 ^ v7);                                                                          \
    }
VS_KERNEL(k_v_cndmask_sgpr, I_CNDM_SG)
VS_KERNEL(k_v_and_sgpr, I_AND_SG)
// v_cndmask_b32 reading VCC, with VCC written by the scalar unit at the head of every iteration (k_v_cndmask never writes it)
__global__ __launch_bounds__(64) void k_v_cndmask_vcc_set(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {
    uint32_t v0 = threadIdx.x, v1 = v0 + 1, v2 = v0 + 2, v3 = v0 + 3, v4 = v0 + 4, v5 = v0 + 5, v6 = v0 + 6, v7 = v0 + 7;
    const uint32_t va = a + threadIdx.x; const uint64_t sm = ((uint64_t)b << 32) | a;
    BEGIN();
    for (int it = 0; it < iters; it++)
        asm volatile("s_mov_b64 vcc, %9\ns_nop 4\n" R128(I_CNDM) : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7)
                     : "v"(va), "s"(sm) : "vcc", "memory");
    END(0u, v0 ^ v1 ^ v2 ^ v3 ^ v4 ^ v5 ^ v6 ^ v7);
}

// ---- other shapes of the VCC select (the probes above are one shape: destination = first source, VCC never written by a compare) ----
// the short form with a destination distinct from both sources
#define I_CNDM_D(k) "v_cndmask_b32_e32 %" #k ", %8, %9, vcc\n"
V_KERNEL(k_v_cndmask_dst, I_CNDM_D, "memory")
// the VOP3 encoding with vcc named as the mask
#define I_CNDM_E64(k) "v_cndmask_b32_e64 %" #k ", %" #k ", %8, vcc\n"
V_KERNEL(k_v_cndmask_e64_vcc, I_CNDM_E64, "memory")
// the short form with VCC written by a vector compare at the head of every iteration (as the compiler's code does: v_cmp, then the selects)
__global__ __launch_bounds__(64) void k_v_cndmask_vcmp(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {
    uint32_t v0 = threadIdx.x, v1 = v0 + 1, v2 = v0 + 2, v3 = v0 + 3, v4 = v0 + 4, v5 = v0 + 5, v6 = v0 + 6, v7 = v0 + 7;
    const uint32_t va = a + threadIdx.x, vb = b ^ threadIdx.x;
    BEGIN();
    for (int it = 0; it < iters; it++)
        asm volatile("v_cmp_lt_u32_e32 vcc, %0, %9\n" R128(I_CNDM) : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7)
                     : "v"(va), "v"(vb) : "vcc", "memory");
    END(0u, v0 ^ v1 ^ v2 ^ v3 ^ v4 ^ v5 ^ v6 ^ v7);
}
// (a kernel whose iteration is a given string of 128 instructions on the same operands as V_KERNEL's)
#define V_KERNEL_STR(NAME, BODY, ...)                                                                                            \
    __global__ __launch_bounds__(64) void NAME(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {                   \
        uint32_t v0 = threadIdx.x, v1 = v0 + 1, v2 = v0 + 2, v3 = v0 + 3, v4 = v0 + 4, v5 = v0 + 5, v6 = v0 + 6, v7 = v0 + 7;    \
        const uint32_t va = a + threadIdx.x, vb = b ^ threadIdx.x;                                                               \
        BEGIN();                                                                                                                 \
        for (int it = 0; it < iters; it++)                                                                                       \
            asm volatile(BODY : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7)                   \
                         : "v"(va), "v"(vb) : __VA_ARGS__);                                                                      \
        END(0u, v0 ^ v1 ^ v2 ^ v3 ^ v4 ^ v5 ^ v6 ^ v7);                                                                          \
    }
// one compare into VCC per select, as in a chain of `x = c ? a : b` on different conditions: 64 pairs per iteration
#define I_CMP_CNDM(k) "v_cmp_lt_u32_e32 vcc, %" #k ", %9\nv_cndmask_b32_e32 %" #k ", %" #k ", %8, vcc\n"
#define R64(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I)
V_KERNEL_STR(k_v_cmp_cndmask_pairs, R64(I_CMP_CNDM), "vcc", "memory")
// the short form interleaved 1:1 with independent v_and_b32: selects on accumulators 0..3, ands on 4..7, 64 of each per iteration
#define I_CA(k, j) "v_cndmask_b32_e32 %" #k ", %" #k ", %8, vcc\nv_and_b32 %" #j ", %8, %" #j "\n"
#define CA4 I_CA(0, 4) I_CA(1, 5) I_CA(2, 6) I_CA(3, 7)
#define CA64 CA4 CA4 CA4 CA4 CA4 CA4 CA4 CA4 CA4 CA4 CA4 CA4 CA4 CA4 CA4 CA4
V_KERNEL_STR(k_v_cndmask_and_mix, CA64, "memory")

// 64-bit shift: 8 accumulator pairs
#define I_LSHR64(k) "v_lshrrev_b64 %" #k ", %8, %" #k "\n"
__global__ __launch_bounds__(64) void k_v_lshrrev_b64(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {
    uint64_t v0 = threadIdx.x | ((uint64_t)b << 32), v1 = v0 + 1, v2 = v0 + 2, v3 = v0 + 3, v4 = v0 + 4, v5 = v0 + 5, v6 = v0 + 6, v7 = v0 + 7;
    const uint32_t va = (a + threadIdx.x) & 1u;
    BEGIN();
    for (int it = 0; it < iters; it++)
        asm volatile(R128(I_LSHR64) : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7) : "v"(va) : "memory");
    END(0u, (uint32_t)(v0 ^ v1 ^ v2 ^ v3 ^ v4 ^ v5 ^ v6 ^ v7));
}
// compare into a scalar register pair, lane read into a scalar register: 4 scalar results %0..%3, vector inputs %4 %5
#define I_CMPSG(k) "v_cmp_eq_u32_e64 %" #k ", %4, %5\n"
__global__ __launch_bounds__(64) void k_v_cmp_sgpr(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {
    uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    const uint32_t va = a + threadIdx.x, vb = b ^ threadIdx.x;
    BEGIN();
    for (int it = 0; it < iters; it++) asm volatile(S128(I_CMPSG) : "=s"(s0), "=s"(s1), "=s"(s2), "=s"(s3) : "v"(va), "v"(vb) : "memory");
    END(0u, (uint32_t)(s0 ^ s1 ^ s2 ^ s3));
}
#define I_RDLANE(k) "v_readlane_b32 %" #k ", %4, 5\n"
__global__ __launch_bounds__(64) void k_v_readlane(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    const uint32_t va = a + threadIdx.x, vb = b;
    BEGIN();
    for (int it = 0; it < iters; it++) asm volatile(S128(I_RDLANE) : "=s"(s0), "=s"(s1), "=s"(s2), "=s"(s3) : "v"(va), "v"(vb) : "memory");
    END(0u, s0 ^ s1 ^ s2 ^ s3);
}

// ---- scalar classes: 4 accumulators %0..%3, scalar inputs %4 %5 ----
#define I_SAND64(k) "s_and_b64 %" #k ", %" #k ", %4\n"
#define I_SCSEL64(k) "s_cselect_b64 %" #k ", %4, %" #k "\n"
#define I_SBITSET(k) "s_bitset1_b64 %" #k ", %5\n"
#define S64_KERNEL(NAME, I)                                                                                                       \
    __global__ __launch_bounds__(64) void NAME(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {                    \
        uint64_t s0 = a, s1 = a + 1u, s2 = a + 2u, s3 = a + 3u;                                                                    \
        const uint64_t sa = ((uint64_t)b << 32) | a; const uint32_t sb = b & 63u;                                                  \
        BEGIN();                                                                                                                  \
        for (int it = 0; it < iters; it++) asm volatile(S128(I) : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : "s"(sa), "s"(sb) : "scc", "memory"); \
        END(0u, (uint32_t)(s0 ^ s1 ^ s2 ^ s3));                                                                                    \
    }
S64_KERNEL(k_s_and_b64, I_SAND64)
S64_KERNEL(k_s_cselect_b64, I_SCSEL64)
S64_KERNEL(k_s_bitset1_b64, I_SBITSET)
#define I_SADD(k) "s_add_i32 %" #k ", %" #k ", %4\n"
#define I_SBCNT(k) "s_bcnt1_i32_b64 %" #k ", %5\n"
__global__ __launch_bounds__(64) void k_s_add_i32(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {
    uint32_t s0 = a, s1 = a + 1u, s2 = a + 2u, s3 = a + 3u;
    const uint64_t sb = ((uint64_t)b << 32) | a;
    BEGIN();
    for (int it = 0; it < iters; it++) asm volatile(S128(I_SADD) : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : "s"(b), "s"(sb) : "scc", "memory");
    END(0u, s0 ^ s1 ^ s2 ^ s3);
}
__global__ __launch_bounds__(64) void k_s_bcnt1_i32_b64(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {
    uint32_t s0 = a, s1 = a + 1u, s2 = a + 2u, s3 = a + 3u;
    const uint64_t sb = ((uint64_t)b << 32) | a;
    BEGIN();
    for (int it = 0; it < iters; it++) asm volatile(S128(I_SBCNT) : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : "s"(b), "s"(sb) : "scc", "memory");
    END(0u, s0 ^ s1 ^ s2 ^ s3);
}
// branches on SCC: taken (over an s_nop that never runs) and not taken; SCC is set once per iteration
#define I_BR_TAKEN(k) "s_cbranch_scc1 1f\ns_nop 0\n1:\n"
#define I_BR_NOT(k)   "s_cbranch_scc0 1f\n1:\n"
#define BR_KERNEL(NAME, I)                                                                                                        \
    __global__ __launch_bounds__(64) void NAME(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {                    \
        BEGIN();                                                                                                                  \
        for (int it = 0; it < iters; it++) asm volatile("s_cmp_eq_u32 0, 0\n" S128(I) : : : "scc", "memory");                      \
        END(0u, a ^ b);                                                                                                            \
    }
BR_KERNEL(k_s_cbranch_taken, I_BR_TAKEN)
BR_KERNEL(k_s_cbranch_not_taken, I_BR_NOT)

// ---- 1:1 mixes of v_and_b32 and s_and_b64 ----
#define I_MIX(k) "v_and_b32 %" #k ", %9, %" #k "\ns_and_b64 %8, %8, %10\n"
#define M64(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I) R8(I)
__global__ __launch_bounds__(64) void k_mix_one_wave(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {
    uint32_t v0 = threadIdx.x, v1 = v0 + 1, v2 = v0 + 2, v3 = v0 + 3, v4 = v0 + 4, v5 = v0 + 5, v6 = v0 + 6, v7 = v0 + 7;
    const uint32_t va = a + threadIdx.x;
    uint64_t s0 = a; const uint64_t sa = ((uint64_t)b << 32) | a;
    BEGIN();
    for (int it = 0; it < iters; it++)                      // 64 vector + 64 scalar = PER_ITER wave-instructions
        asm volatile(M64(I_MIX) : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7), "+s"(s0) : "v"(va), "s"(sa) : "scc", "memory");
    END(0u, v0 ^ v1 ^ v2 ^ v3 ^ v4 ^ v5 ^ v6 ^ v7 ^ (uint32_t)s0);
}
__global__ __launch_bounds__(64) void k_mix_two_waves(Stamp *st, uint32_t *sink, uint32_t a, uint32_t b, int iters) {
    uint32_t v0 = threadIdx.x, v1 = v0 + 1, v2 = v0 + 2, v3 = v0 + 3, v4 = v0 + 4, v5 = v0 + 5, v6 = v0 + 6, v7 = v0 + 7;
    const uint32_t va = a + threadIdx.x, vb = b ^ threadIdx.x;
    uint64_t s0 = a, s1 = a + 1u, s2 = a + 2u, s3 = a + 3u; const uint64_t sa = ((uint64_t)b << 32) | a; const uint32_t sb = b & 63u;
    const uint32_t role = hw_id() & 1u;                     // odd wave slots of a SIMD: the scalar stream
    BEGIN();
    if (role) { for (int it = 0; it < iters; it++) asm volatile(S128(I_SAND64) : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) : "s"(sa), "s"(sb) : "scc", "memory"); }
    else { for (int it = 0; it < iters; it++) asm volatile(R128(I_AND) : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7) : "v"(va), "v"(vb) : "memory"); }
    END(role, v0 ^ v1 ^ v2 ^ v3 ^ v4 ^ v5 ^ v6 ^ v7 ^ (uint32_t)(s0 ^ s1 ^ s2 ^ s3));
}

typedef void (*kern_t)(Stamp *, uint32_t *, uint32_t, uint32_t, int);
struct Probe { const char *name; const char *unit; kern_t k; };
static const Probe PROBES[] = {
    {"v_and_b32", "vector", k_v_and}, {"v_perm_b32", "vector", k_v_perm}, {"v_alignbyte_b32", "vector", k_v_alignbyte},
    {"v_mad_u32_u24", "vector", k_v_mad_u32_u24}, {"v_cndmask_b32 vcc (never written)", "vector", k_v_cndmask}, {"v_cndmask_b32 vcc (set per iteration)", "vector", k_v_cndmask_vcc_set},
    {"v_cndmask_b32 sgpr pair mask", "vector", k_v_cndmask_sgpr}, {"v_and_b32 sgpr operand", "vector", k_v_and_sgpr}, {"v_lshrrev_b64", "vector", k_v_lshrrev_b64},
    {"v_ffbl_b32", "vector", k_v_ffbl}, {"v_cmp_eq_u32 vcc", "vector", k_v_cmp_vcc}, {"v_cmp_eq_u32 sgpr pair", "vector", k_v_cmp_sgpr},
    {"v_readlane_b32", "vector", k_v_readlane},
    {"v_cndmask_b32_e32 vcc, destination distinct from both sources", "vector", k_v_cndmask_dst}, {"v_cndmask_b32_e64 with vcc named as the mask", "vector", k_v_cndmask_e64_vcc},
    {"v_cndmask_b32_e32 vcc (set by one v_cmp per iteration)", "vector", k_v_cndmask_vcmp}, {"v_cmp_lt_u32 vcc + v_cndmask_b32_e32 vcc, pairs", "vector", k_v_cmp_cndmask_pairs},
    {"v_cndmask_b32_e32 vcc + v_and_b32, 1:1", "vector", k_v_cndmask_and_mix},
    {"s_and_b64", "scalar", k_s_and_b64}, {"s_add_i32", "scalar", k_s_add_i32}, {"s_bcnt1_i32_b64", "scalar", k_s_bcnt1_i32_b64},
    {"s_cselect_b64", "scalar", k_s_cselect_b64}, {"s_bitset1_b64", "scalar", k_s_bitset1_b64},
    {"s_cbranch_scc taken", "branch", k_s_cbranch_taken}, {"s_cbranch_scc not taken", "branch", k_s_cbranch_not_taken},
    {"v_and_b32 + s_and_b64, one wave", "mix", k_mix_one_wave}, {"v_and_b32 | s_and_b64, two waves of a SIMD", "mix", k_mix_two_waves},
};

static double median(std::vector<double> v) { if (v.empty()) return 0.0; std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char **argv) {
    const char *out = argc > 1 ? argv[1] : "issue_rates.json";
    const int iters = argc > 2 ? atoi(argv[2]) : 8000;
    hipDeviceProp_t pr; CK(hipGetDeviceProperties(&pr, 0));
    const int cus = pr.multiProcessorCount;
    const size_t lds_cu = pr.maxSharedMemoryPerMultiProcessor ? pr.maxSharedMemoryPerMultiProcessor : 160u << 10;
    const int WAVES[] = {1, 2, 4, 6};
    const unsigned max_grid = (unsigned)cus * 4u * 6u;
    Stamp *d_st; uint32_t *d_sink;
    CK(hipMalloc(&d_st, max_grid * sizeof(Stamp))); CK(hipMalloc(&d_sink, (size_t)max_grid * 64 * 4));
    std::vector<Stamp> h(max_grid);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::string js = "{\n \"device\": \"" + std::string(pr.gcnArchName) + "\", \"cus\": " + std::to_string(cus) + ", \"iters\": " + std::to_string(iters) +
                     ", \"instructions_per_iteration\": " + std::to_string(PER_ITER) + ",\n \"probes\": [\n";
    bool first = true;
    for (const Probe &p : PROBES) {
        for (int w : WAVES) {
            const unsigned grid = (unsigned)cus * 4u * (unsigned)w;
            const size_t lds = (lds_cu / (4u * (size_t)w)) & ~(size_t)255;                // 4 w workgroups fill a CU's LDS: no more fit
            CK(hipFuncSetAttribute((const void *)p.k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            float best = 1e30f;
            for (int rep = 0; rep < 4; rep++) {                                              // rep 0 warms up
                CK(hipEventRecord(e0, 0));
                hipLaunchKernelGGL(p.k, dim3(grid), dim3(64), lds, 0, d_st, d_sink, 0x01234567u, 0x89abcdefu, iters);
                CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                if (rep && ms < best) best = ms;
            }
            CK(hipMemcpy(h.data(), d_st, grid * sizeof(Stamp), hipMemcpyDeviceToHost));
            std::vector<double> cyc[2], clk;
            unsigned simd[4] = {0, 0, 0, 0}, roles[2] = {0, 0};
            uint64_t rmin = ~0ull, rmax = 0;
            for (unsigned i = 0; i < grid; i++) {
                const Stamp &s = h[i];
                cyc[s.role & 1].push_back((double)(s.c1 - s.c0) / ((double)iters * PER_ITER));
                if (s.r1 > s.r0) clk.push_back((double)(s.c1 - s.c0) / (double)(s.r1 - s.r0) * 0.1);
                simd[(s.hwid >> 4) & 3]++; roles[s.role & 1]++;
                rmin = std::min(rmin, s.r0); rmax = std::max(rmax, s.r1);
            }
            const double insts = (double)grid * iters * PER_ITER;
            const double rate = insts / ((double)best * 1e6) / cus;                          // wave-instructions per ns per CU
            const double span_ms = (double)(rmax - rmin) * 1e-5;                             // first stamp to last, 100 MHz ticks
            char line[1024];
            snprintf(line, sizeof line,
                     "  %s{\"class\": \"%s\", \"unit\": \"%s\", \"waves_per_simd\": %d, \"ms\": %.4f, \"all_waves_span_ms\": %.4f, \"wave_insts_per_ns_per_cu\": %.4f, "
                     "\"cycles_per_inst_one_wave\": %.3f, \"cycles_per_inst_one_wave_role1\": %.3f, \"clock_ghz\": %.3f, \"wave_insts_per_cycle_per_cu\": %.3f, "
                     "\"waves_by_simd\": [%u, %u, %u, %u], \"waves_by_role\": [%u, %u]}",
                     first ? "" : ",", p.name, p.unit, w, best, span_ms, rate, median(cyc[0]), median(cyc[1]), median(clk),
                     median(clk) > 0 ? rate / median(clk) : 0.0, simd[0], simd[1], simd[2], simd[3], roles[0], roles[1]);
            js += line; js += "\n"; first = false;
            printf("%-44s W=%d  %8.3f ms  %7.3f inst/ns/CU  %6.2f cyc/inst/wave  %5.3f GHz  %5.2f inst/cyc/CU\n", p.name, w, best, rate, median(cyc[0]), median(clk),
                   median(clk) > 0 ? rate / median(clk) : 0.0);
            fflush(stdout);
        }
    }
    js += " ]\n}\n";
    FILE *f = fopen(out, "w"); if (!f) { perror(out); return 2; }
    fputs(js.c_str(), f); fclose(f);
    CK(hipFree(d_st)); CK(hipFree(d_sink));
    return 0;
}
