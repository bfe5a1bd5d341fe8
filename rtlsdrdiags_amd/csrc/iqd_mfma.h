// Device-only building blocks shared by the chain kernels that run their first FIR stage on the matrix cores
// (v_mfma_i32_16x16x64_i8): the byte-level front end and the squelch magnitude.  gfx950 only (no host twin).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_prims.h"

namespace iqd {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned short us2 __attribute__((ext_vector_type(2)));

typedef float v2f __attribute__((ext_vector_type(2)));
// x * (s, s) as ONE v_pk_mul_f32 with the constant pair in scalar registers (left to itself the compiler multiplies the
// halves one by one: a literal does not fit a packed instruction)
__device__ __forceinline__ v2f pk_mul_s(v2f x, uint64_t s_pair)
{
    v2f r;
    asm("v_pk_mul_f32 %0, %1, %2" : "=v"(r) : "v"(x), "s"(s_pair));
    return r;
}

// ---- small device helpers -----------------------------------------------------------------------
// byte B of x replaced by its two's-complement negation, the other bytes kept (v_sub_u32_sdwa): int8
// wrap, so -(-128) stays -128 like the reference's rotation (IqDataProcessor.cc:594-607)
#define ST_NEG_BYTE(x, B)                                                                                     \
    asm("v_sub_u32_sdwa %0, %1, %0 dst_sel:BYTE_" #B " dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:BYTE_" #B \
        : "+v"(x) : "v"(zero))

// raw offset-binary bytes of 8 samples -> signed bytes with the rotation's SIGNS applied in place (which
// byte feeds which rail is folded into the tap matrices).  +Fs/4: I' = {I0,-Q1,-I2,Q3}, Q' = {Q0,I1,-Q2,-I3};
// -Fs/4: I' = {I0,Q1,-I2,-Q3}, Q' = {Q0,-I1,-Q2,I3} (IqDataProcessor.cc:567-611).
template <int ROT>
__device__ __forceinline__ uint4 st_front(uint4 raw, uint32_t zero)
{
    uint32_t d[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int h = 0; h < 4; h += 2) {
        uint32_t d0 = d[h], d1 = d[h + 1];
        if (ROT == 0) {
            d0 ^= 0x80808080u;
            d1 ^= 0x80808080u;
        } else if (ROT > 0) {
            d0 = (d0 ^ 0x7f808080u) + 0x01000000u;   // byte 3 (Q1): ~s + 1, the carry leaves the register
            d1 ^= 0x80808080u;
            ST_NEG_BYTE(d1, 0);
            ST_NEG_BYTE(d1, 1);
            ST_NEG_BYTE(d1, 2);
        } else {
            d0 ^= 0x80808080u;
            ST_NEG_BYTE(d0, 2);
            d1 = (d1 ^ 0x7f808080u) + 0x01000000u;   // byte 3 (Q3)
            ST_NEG_BYTE(d1, 0);
            ST_NEG_BYTE(d1, 1);
        }
        d[h] = d0;
        d[h + 1] = d1;
    }
    return uint4{d[0], d[1], d[2], d[3]};
}

// sum over the 2 samples of a dword of RAW bytes (offset binary I0 Q0 I1 Q1) of max(|I|,|Q|) + min(|I|,|Q|)/2, added into two
// 16-bit lanes of acc (SignalDetector.cc:227-247), with ONE quad-SAD: the dword's bytes are put in the order I0 I1 Q0 Q1
// (v_perm_b32) and v_mqsad_pk_u16_u8 against the reference 0x00000080 - only its byte 0 counts, at the four byte positions in
// turn - leaves |I0 - 128|, |I1 - 128| as the halves of one register and |Q0 - 128|, |Q1 - 128| of the next: six instructions per
// dword (the quad-SAD issues at a quarter of the rate, tools/ubench).
__device__ __forceinline__ uint32_t st_mag_raw_dword_q(uint32_t raw, uint32_t acc)
{
    const uint32_t p = __builtin_amdgcn_perm(raw, raw, 0x03010200u);
    uint32_t upper = 0;
    upper = __builtin_nondeterministic_value(upper);             // (bytes 4-6 of the source are compared with masked reference bytes)
    const uint64_t r = __builtin_amdgcn_mqsad_pk_u16_u8((uint64_t)p | ((uint64_t)upper << 32), 0x00000080u, 0ull);
    const us2 a = __builtin_bit_cast(us2, (uint32_t)r), b = __builtin_bit_cast(us2, (uint32_t)(r >> 32));
    const us2 mx = __builtin_elementwise_max(a, b), mn = __builtin_elementwise_min(a, b);
    return acc + __builtin_bit_cast(uint32_t, mx) + __builtin_bit_cast(uint32_t, (us2)(mn >> 1));
}
// 8 raw samples (one lane's 16 bytes of a piece) added into the two 16-bit partial sums of acc
__device__ __forceinline__ uint32_t st_mag_raw_chunk(const uint4 &raw, uint32_t acc)
{
    acc = st_mag_raw_dword_q(raw.x, acc);
    acc = st_mag_raw_dword_q(raw.y, acc);
    acc = st_mag_raw_dword_q(raw.z, acc);
    return st_mag_raw_dword_q(raw.w, acc);
}

// ---- input prefetch of the streaming kernels ----
// A 16-byte global load the compiler does not track, and the matching wait.  With ordinary loads the compiler's
// own s_waitcnt placement joins the loop's entry and back edge conservatively (vmcnt(0) at the header, i.e. a wait
// for the load issued one piece ago) and hands buffers on with register moves that wait for the youngest load;
// a P wave then pays a trip to HBM per piece however many pieces it asked for in advance.  Loads return in order,
// so "at most N younger loads outstanding" is exactly "this one has arrived"; other memory operations issued in
// between (magnitude atomics) only make the wait stricter.  Nothing that is not inlined may be called while such loads
// are in flight: a callee uses registers as it pleases (tried: a noinline helper in the piece loop corrupted everything).
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4u gload16_untracked(const void *p)
{
    v4u r;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r) : "v"(p));
    return r;
}
// (In place, on the variable the load was issued into: handing the value to the wait by copy invites the compiler to
// make that copy - of registers still in flight - in front of the wait.  tools/isa_lint.py checks the generated code
// for exactly this.)
template <int N_YOUNGER>
__device__ __forceinline__ void gload_wait(v4u &r)
{
    asm volatile("s_waitcnt vmcnt(%1) ; arrived %0" : "+v"(r) : "n"(N_YOUNGER));   // (the comment is for tools/isa_lint.py)
}
// the same with a count that is only known after unrolling (folds to one s_waitcnt)
__device__ __forceinline__ void gload_wait_n(v4u &r, int n_younger)
{
    switch (n_younger) {
    case 1: gload_wait<1>(r); break;
    case 2: gload_wait<2>(r); break;
    case 3: gload_wait<3>(r); break;
    case 4: gload_wait<4>(r); break;
    case 5: gload_wait<5>(r); break;
    case 6: gload_wait<6>(r); break;
    case 7: gload_wait<7>(r); break;
    case 8: gload_wait<8>(r); break;
    case 9: gload_wait<9>(r); break;
    case 10: gload_wait<10>(r); break;
    case 11: gload_wait<11>(r); break;
    default: gload_wait<0>(r); break;
    }
}
__device__ __forceinline__ uint4 as_uint4(v4u r) { return uint4{r.x, r.y, r.z, r.w}; }
__device__ __forceinline__ uint32_t gload4_untracked(const void *p)
{
    uint32_t r;
    asm volatile("global_load_dword %0, %1, off" : "=v"(r) : "v"(p));
    return r;
}
template <int N_YOUNGER>
__device__ __forceinline__ void gload_wait(uint32_t &r)
{
    asm volatile("s_waitcnt vmcnt(%1) ; arrived %0" : "+v"(r) : "n"(N_YOUNGER));
}

// ---- producer / consumer plumbing of the streaming kernels (waves of one workgroup talking through LDS rings) ----
// (through the LDS address space: on the generic pointer this is a flat_load, which travels the vector-memory path
// as well and is waited for with vmcnt(0) - i.e. together with every input load the wave has in flight)
__device__ __forceinline__ uint32_t lds_load_relaxed(const uint32_t *p)
{
    const __attribute__((address_space(3))) uint32_t *q = (const __attribute__((address_space(3))) uint32_t *)(uintptr_t)(uint32_t)(uintptr_t)p;
    return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// lane 0 adds `n` (1 unless said otherwise) to an LDS word (exec is all ones wherever this is used); the plain HIP form costs
// a dozen instructions of "which lane is first" bookkeeping per call
__device__ __forceinline__ void lds_signal(const uint32_t *p, uint32_t n = 1u)
{
    const uint32_t addr = (uint32_t)(uintptr_t)p;
    asm volatile("s_mov_b64 exec, 1\n\tds_add_u32 %0, %1\n\ts_mov_b64 exec, -1" :: "v"(addr), "v"(n) : "memory");
}

// The same two for a wave that keeps the LDS byte address of its ring's sync words in a vector register (st_iir_wave): the word
// OFF bytes behind it, the constant in the instruction's offset field - through a uniform pointer the address is a scalar that
// has to be moved into a vector register in front of every look.  lds_word_uniform: the word is the same in every lane, so the
// value goes to the scalar unit (one v_readfirstlane_b32) and whatever is tested on it is scalar arithmetic and a scalar branch.
__device__ __forceinline__ uint32_t lds_word_uniform(uint32_t base, uint32_t off)
{
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_load_relaxed((const uint32_t *)(uintptr_t)(base + off)));
}
template <int OFF>
__device__ __forceinline__ void lds_signal_at(uint32_t base, uint32_t n = 1u)
{
    asm volatile("s_mov_b64 exec, 1\n\tds_add_u32 %0, %1 offset:%2\n\ts_mov_b64 exec, -1" :: "v"(base), "v"(n), "n"(OFF) : "memory");
}

// byte offset of granule q (4 samples) of ring row j inside a slot: XOR swizzle, conflict-free for the
// P waves' ds_write_b128 and the IIR lanes' ds_read_b128
__device__ __forceinline__ uint32_t st_slot_off(uint32_t j, uint32_t q) { return j * 64u + ((q ^ ((j >> 2) & 3u)) << 4); }


}  // namespace iqd
