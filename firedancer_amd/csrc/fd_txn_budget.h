/* firedancer_amd/csrc/fd_txn_budget.h -- a transaction's compute budget and
   fee (include/fd_txn_amd.h, "Compute budget"): what the reference's
   fd_compute_budget_program_{init,parse,finalize}
   (src/ballet/pack/fd_compute_budget_program.h:71-204) make of the
   instructions addressed to ComputeBudget111111111111111111111111111111, as
   one 24-byte fd_txn_amd_budget_t per transaction.

   Two parts.  The first is the rule's arithmetic over byte pointers: the
   program address compare, one parse step, the finalize and the record's
   three 64-bit words.  The host rule (fd_ed25519_host.cpp, plain C++) and the
   kernel below both compile these functions, so the CPU tests exercise the
   arithmetic the GPU runs.  Fields are assembled from byte loads: instruction
   data has any alignment.  The second part, the kernel, is compiled only
   where fd_txn_dev.h was included first (fd_txn_kernels.hip).

     k_txn_budget  one lane per transaction, behind k_txn_parse: footprint 0
                   gives _NOPARSE; otherwise the lane walks the payload's
                   instructions with fd_txn_dev.h's checked cursor (`room`
                   before every read: whatever the planes hold, nothing
                   outside [payload + off, + sz) is read, and a bound that
                   fails ends in _NOPARSE), runs the step on every
                   instruction whose program address is the id, and stores
                   the record as three 8-byte vector stores.  No atomics, no
                   spinning, no workgroup waits for another.

   The loop.  Lanes of one wave have 1 to 355 instructions (21789 at 65535
   bytes), so the wave runs the longest lane's trip count whatever the body
   holds; the body is therefore kept to what every instruction needs, four
   loads in the usual case: the program index, the two counts (one byte each
   below 128) and the first word of the program's address.  Only an address
   whose first word is the id's goes on to the other seven words and the
   step, and a lane that has rejected leaves the loop.  A "word" is written
   as four byte loads (fd_amd_budget_ld32); in the gfx950 code object hipcc
   makes one global_load_dword of each, and one dwordx4 and one dwordx3 of
   the address's other seven (read off the disassembly of k_txn_budget: 35
   VGPRs, no scratch; unaligned dword loads are legal there).  What the walk
   of a 355-instruction lane costs has not been measured. */
#ifndef FD_TXN_BUDGET_RULE_H
#define FD_TXN_BUDGET_RULE_H

#include <stdint.h>

#if defined(__HIP__)
#define FD_BUDGET_FN static inline __host__ __device__
#else
#define FD_BUDGET_FN static inline
#endif

/* fd_txn_amd_budget_t's status and flags (include/fd_txn_amd.h spells them
   FD_TXN_AMD_BUDGET_*; fd_ed25519_engine.cpp asserts the two agree) */
#define FD_AMD_BUDGET_OK      0u
#define FD_AMD_BUDGET_INVALID 1u
#define FD_AMD_BUDGET_NOPARSE 2u
#define FD_AMD_BUDGET_F_CU    0x01u   /* fd_compute_budget_program.h:29-32 */
#define FD_AMD_BUDGET_F_FEE   0x02u
#define FD_AMD_BUDGET_F_HEAP  0x04u
#define FD_AMD_BUDGET_F_TOTAL 0x08u

/* the walk's state: fd_compute_budget_program_state_t's fields */
typedef struct {
  uint64_t price;      /* micro_lamports_per_cu */
  uint32_t cu;         /* compute_units */
  uint32_t total_fee;
  uint32_t heap;       /* heap_size */
  uint32_t flags;
  uint32_t cnt;        /* compute_budget_instr_cnt */
} fd_amd_budget_state_t;

FD_BUDGET_FN uint32_t
fd_amd_budget_ld32( uint8_t const * p ) {
  return (uint32_t)p[0] | ( (uint32_t)p[1] << 8 ) | ( (uint32_t)p[2] << 16 ) | ( (uint32_t)p[3] << 24 );
}

/* The id, base58 ComputeBudget111111111111111111111111111111, as eight
   little-endian words: 03 06 46 6f e5 21 17 32 ff ec ad ba 72 c3 9b e7
   bc 8c e5 bb c5 f7 12 6b 2c 43 9b 3a 40 00 00 00
   (fd_compute_budget_program.h:18-21). */
#define FD_AMD_BUDGET_ID_W0 0x6f460603u

/* The first word of the 32-byte address at a: most addresses end here. */
FD_BUDGET_FN int
fd_amd_budget_id_head( uint8_t const * a ) { return fd_amd_budget_ld32( a ) == FD_AMD_BUDGET_ID_W0; }

/* The other seven, for an address whose first word matched. */
FD_BUDGET_FN int
fd_amd_budget_id_tail( uint8_t const * a ) {
  uint32_t d = ( fd_amd_budget_ld32( a +  4 ) ^ 0x321721e5u ) | ( fd_amd_budget_ld32( a +  8 ) ^ 0xbaadecffu ) |
               ( fd_amd_budget_ld32( a + 12 ) ^ 0xe79bc372u ) | ( fd_amd_budget_ld32( a + 16 ) ^ 0xbbe58cbcu ) |
               ( fd_amd_budget_ld32( a + 20 ) ^ 0x6b12f7c5u ) | ( fd_amd_budget_ld32( a + 24 ) ^ 0x3a9b432cu ) |
               ( fd_amd_budget_ld32( a + 28 ) ^ 0x00000040u );
  return !d;
}

/* One compute-budget instruction, data[0, sz): fd_compute_budget_program_parse
   (:81-126).  Returns 1 and updates s, or 0: the transaction is _INVALID and
   s is not to be used (the heap value is in it when the granularity check
   fails, as in the reference: the callers zero the record). */
FD_BUDGET_FN int
fd_amd_budget_step( fd_amd_budget_state_t * s, uint8_t const * data, uint32_t sz ) {
  if( sz < 5u ) return 0;                                   /* :85, before the discriminant */
  uint32_t const kind = data[0], a = fd_amd_budget_ld32( data + 1 );
  uint32_t need, clash, set;
  switch( kind ) {
    case 0u:  need = 9u; clash = FD_AMD_BUDGET_F_CU | FD_AMD_BUDGET_F_FEE;                         /* RequestUnitsDeprecated */
              set  = FD_AMD_BUDGET_F_CU | FD_AMD_BUDGET_F_FEE | FD_AMD_BUDGET_F_TOTAL; break;
    case 1u:  need = 5u; clash = set = FD_AMD_BUDGET_F_HEAP; break;                                /* RequestHeapFrame */
    case 2u:  need = 5u; clash = set = FD_AMD_BUDGET_F_CU;   break;                                /* SetComputeUnitLimit */
    case 3u:  need = 9u; clash = set = FD_AMD_BUDGET_F_FEE;  break;                                /* SetComputeUnitPrice */
    default:  return 0;
  }
  if( sz != need || ( s->flags & clash ) ) return 0;
  uint32_t const b = need == 9u ? fd_amd_budget_ld32( data + 5 ) : 0u;
  if(      kind == 0u ) { s->cu = a; s->total_fee = b; }
  else if( kind == 1u ) { s->heap = a; if( a & 1023u ) return 0; }                                  /* :102-103 */
  else if( kind == 2u ) s->cu = a;
  else                  s->price = (uint64_t)a | ( (uint64_t)b << 32 );
  s->flags |= set;
  s->cnt++;
  return 1;
}

/* fd_compute_budget_program_finalize (:139-204) for a transaction of
   instr_cnt instructions: *compute, and the rewards.  The limit is a 64-bit
   value (the default, 200000 per instruction that is not a budget
   instruction, passes 2^32 from 21475 of them up); *compute is its low half,
   the fee uses all of it.  The fee is min( 2^64 - 1, ceil( limit * price /
   10^6 ) ) in the reference's split form, without 128-bit arithmetic: limit
   = ch 10^6 + cl, price = ph 10^6 + pl, so the quotient is ch ph 10^6 +
   ch pl + cl ph + ceil( cl pl / 10^6 ); ch ph above floor( (2^64 - 1) / 10^6
   ) saturates, and so does a wrap of the last addition. */
FD_BUDGET_FN uint64_t
fd_amd_budget_finalize( fd_amd_budget_state_t const * s, uint32_t instr_cnt, uint32_t * compute ) {
  uint64_t const M = 1000000UL;
  uint64_t const limit = ( s->flags & FD_AMD_BUDGET_F_CU ) ? (uint64_t)s->cu : (uint64_t)( instr_cnt - s->cnt ) * 200000UL;
  *compute = (uint32_t)limit;
  if( s->flags & FD_AMD_BUDGET_F_TOTAL ) return (uint64_t)s->total_fee;
  uint64_t const ch = limit / M, cl = limit % M, ph = s->price / M, pl = s->price % M;
  uint64_t hh = ch * ph;
  if( hh > 0xFFFFFFFFFFFFFFFFUL / M ) return 0xFFFFFFFFFFFFFFFFUL;
  hh *= M;
  uint64_t const fee = hh + ( ch*pl + cl*ph + ( cl*pl + M - 1UL ) / M );
  return fee < hh ? 0xFFFFFFFFFFFFFFFFUL : fee;
}

/* The record as its three little-endian 64-bit words: rewards | compute,
   heap_sz | flags, cb_instr_cnt, status.  Anything but _OK is all zeros
   beside the status. */
FD_BUDGET_FN void
fd_amd_budget_record( uint64_t w[3], fd_amd_budget_state_t const * s, uint32_t instr_cnt, uint32_t status ) {
  if( status != FD_AMD_BUDGET_OK ) { w[0] = 0UL; w[1] = 0UL; w[2] = (uint64_t)status << 32; return; }
  uint32_t compute;
  w[0] = fd_amd_budget_finalize( s, instr_cnt, &compute );
  w[1] = (uint64_t)compute | ( (uint64_t)s->heap << 32 );
  w[2] = (uint64_t)( s->flags & 0xFFFFu ) | ( (uint64_t)( s->cnt & 0xFFFFu ) << 16 ) | ( (uint64_t)status << 32 );
}

#endif /* FD_TXN_BUDGET_RULE_H */

#if defined(FD_TXN_DEV_H) && !defined(FD_TXN_BUDGET_KERNEL_H)
#define FD_TXN_BUDGET_KERNEL_H

/* The walk of one payload that k_txn_parse accepted: the status, the state
   and the instruction count.  Every read is inside [p, p + sz): the cursor's
   room() comes first, and an address is compared only for a program index
   below the account count, whose 32 nacct bytes were checked as one range. */
__device__ inline uint32_t
txn_budget_walk( uint8_t const * p, uint32_t sz, fd_amd_budget_state_t * st, uint32_t * ninstr_out ) {
  fd_txn_dev::cur_t c = { p, sz, 0u };
  uint32_t const NP = FD_AMD_BUDGET_NOPARSE;
  if( !c.room( 1u ) ) return NP;
  uint32_t const nsig = c.b( c.at++ );
  if( !c.room( 64u*nsig ) ) return NP;
  c.at += 64u*nsig;
  if( !c.room( 1u ) ) return NP;
  uint32_t const hdr = ( c.b( c.at++ ) & 0x80u ) ? 3u : 2u;   /* v0: the count, then the two readonly counts */
  if( !c.room( hdr ) ) return NP;
  c.at += hdr;
  uint32_t nacct, ninstr;
  if( !c.cu16( &nacct ) ) return NP;
  if( !c.room( 32u*nacct ) ) return NP;
  uint32_t const acct_off = c.at;
  c.at += 32u*nacct;
  if( !c.room( 32u ) ) return NP;                             /* the blockhash */
  c.at += 32u;
  if( !c.cu16( &ninstr ) ) return NP;
  for( uint32_t j=0u; j<ninstr; j++ ) {
    if( !c.room( 1u ) ) return NP;
    uint32_t const prog = c.b( c.at++ );
    uint32_t nacc, ndata;
    if( !c.cu16( &nacc ) || !c.room( nacc ) ) return NP;
    c.at += nacc;
    if( !c.cu16( &ndata ) || !c.room( ndata ) ) return NP;
    uint8_t const * const data = p + c.at;
    c.at += ndata;
    if( prog >= nacct ) continue;                             /* a lookup-table account: its address is not in the payload */
    uint8_t const * const a = p + acct_off + 32u*prog;
    if( !fd_amd_budget_id_head( a ) ) continue;
    if( !fd_amd_budget_id_tail( a ) ) continue;
    if( !fd_amd_budget_step( st, data, ndata ) ) return FD_AMD_BUDGET_INVALID;
  }
  *ninstr_out = ninstr;
  return FD_AMD_BUDGET_OK;
}

__global__ void __launch_bounds__(64)
k_txn_budget( uint32_t txn_cnt, uint8_t const * __restrict__ payload, uint32_t const * __restrict__ toff,
              uint32_t const * __restrict__ tsz, uint32_t const * __restrict__ fp, uint64_t * __restrict__ budget ) {
  uint32_t const t = blockIdx.x * 64u + threadIdx.x;
  if( t >= txn_cnt ) return;
  fd_amd_budget_state_t st = { 0UL, 0u, 0u, 0u, 0u, 0u };
  uint32_t ninstr = 0u, status = FD_AMD_BUDGET_NOPARSE;
  if( fp[t] ) status = txn_budget_walk( payload + toff[t], tsz[t], &st, &ninstr );
  uint64_t w[3];
  fd_amd_budget_record( w, &st, ninstr, status );
  uint64_t * const o = budget + 3UL*t;
  o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
}

int
fd_amd_launch_txn_budget( uint32_t txn_cnt, uint8_t const * d_payload, uint32_t const * d_toff, uint32_t const * d_tsz,
                          uint32_t const * d_fp, void * d_budget, hipStream_t stream ) {
  if( !txn_cnt ) return 0;
  hipLaunchKernelGGL( k_txn_budget, dim3((txn_cnt + 63u)/64u), dim3(64), 0, stream, txn_cnt, d_payload, d_toff, d_tsz, d_fp,
                      (uint64_t *)d_budget );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

#endif /* FD_TXN_BUDGET_KERNEL_H */
