/* firedancer_amd/csrc/fd_ed25519_frags.h -- k_frag_list, k_frag_check,
   k_frag_verdict: a submission's frags listed by the GPU from the mcache
   lines themselves (fd_ed25519_amd_submit_frags; the rule is "Frag
   submissions" in include/fd_tango_amd.h).

   k_frag_list: one lane per line.  Item i of a submission ( seq0, n ) is line
   (seq0 + i) & (depth - 1) of the mcache, 32 bytes of host memory that a CPU
   may be writing while the kernel runs.  The lane loads the line's word 0
   (seq, sig) and then its word 1 (chunk, sz, ctl, tsorig, tspub), each with
   ONE 16-B load that goes to memory (frag_ld16_sys), in that order; it
   decides the item's status from seq, chunk and sz and writes
     - rec[i], the fd_amd_gather_rec_t k_gather consumes: for a good item the
       three addresses chunk0 + (chunk << 6) + { 0, 32, 96 }, sz - 96 and
       dst = i * stride (stride = round_up( frag_max - 96, 16 ): decided by
       the bound, so no item's offset depends on another line); for an item
       with a nonzero status pub = idle, sig = idle + 32, sz = 0, where idle
       is 96 zero bytes of the slot's own device memory, so the unchanged
       k_gather copies a zero key and signature from the device and nothing
       from the host; msg = idle wherever sz is 0 (k_gather never loads it);
     - status[i], one byte.
   ADDRESS INVARIANT.  Every address in a record either lies in
   [chunk0, chunk0 + data_sz) with its whole range -- ((u64)chunk << 6) + sz
   <= data_sz is checked here, in 64-bit arithmetic: chunk << 6 < 2^38 and
   sz < 2^16, so the sum cannot wrap -- or is the idle block.  chunk0 and
   data_sz are one registered region, translated by the host once per
   submission.  Writes rec[0, n) and status[0, n) and nothing else.  No
   atomics, no spinning, vector stores only.

   Why these loads.  The line is written by fd_mcache_publish: seq - 1, then
   the fields, then seq, and the consumer's protocol is seq, then the fields,
   then (after the frag's bytes were copied) seq again.  Word 0 must therefore
   be read from memory before word 1 is, and neither may be served from a
   cache of this device: `sc0 sc1` is the system-scope form of a global load
   (it bypasses the vector L1 and is not held in L2 for host memory), and the
   s_waitcnt inside each statement completes the first load before the second
   is issued.  The loads are inline asm because no builtin gives a 16-B load
   with those bits on a flat pointer; the compiler counts no load it cannot
   see, so each statement waits for its own (its output is early-clobber and
   valid when the statement ends).  The system-scope acquire fence behind
   them keeps every later load of the lane behind both.

   k_frag_check: the consumer's recheck, ordered behind k_gather by the
   stream: every item whose status is still 0 has its line's seq loaded again
   (8 B, system scope); a mismatch turns the status into FRAG_SEQ.  Writes
   status[] alone.

   k_frag_verdict: the override, behind the verify kernels (behind k_strict
   in strict mode) and ahead of the verdict / tag copy-out, the survivor
   filter and the emit step.  With an mcache it first makes k_frag_check's
   recheck (the engine's one kernel for both: the recheck then also covers
   the time the verify took, which only a producer that ignores flow control
   can tell apart).  For every item with a nonzero status it stores the
   status over the verdict, in d_err and (latency path: the DSM kernel wrote
   the mapped verdicts itself) in m_err, and 0 over the item's tag in the
   workspace's tag plane.  A verdict of FD_AMD_VERDICT_DEVICE stays: the step
   guard marks every verdict of its launch and the host must still see it. */
#ifndef FD_ED25519_FRAGS_H
#define FD_ED25519_FRAGS_H

#define FRAG_HDR (96u)   /* pub 32 | sig 64, then the message */

/* 16 bytes at p (16-aligned, global memory), loaded from memory at system
   scope; complete when the statement ends. */
FD_DEV uint4
frag_ld16_sys( u8 const * p ) {
  gather_w4 w;
  asm volatile( "global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(w) : "v"(p) : "memory" );
  return make_uint4( w.x, w.y, w.z, w.w );
}

FD_DEV u64
frag_ld_seq( u8 const * line ) {
  return __hip_atomic_load( (u64 *)line, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM );
}

__global__ void __launch_bounds__(64)
k_frag_list( u32 n, u8 const * mcache, u64 mask, u64 seq0, u64 chunk0, u64 data_sz, u32 frag_max, u32 stride, u64 idle,
             fd_amd_gather_rec_t * __restrict__ rec, i8 * __restrict__ status ) {
  u32 const i = blockIdx.x * 64u + threadIdx.x;
  if( i >= n ) return;
  u64 const seq = seq0 + (u64)i;                       /* modulo 2^64 */
  u8 const * line = mcache + ((seq & mask) << 5);
  uint4 const w0 = frag_ld16_sys( line );              /* seq | sig */
  uint4 const w1 = frag_ld16_sys( line + 16 );         /* chunk | sz, ctl | tsorig | tspub */
  __builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "" );
  u64 const got = ((u64)w0.y << 32) | w0.x;
  u64 const at = (u64)w1.x << 6;
  u32 const sz = w1.y & 0xFFFFu;
  int st = 0;
  if( got != seq ) st = FD_AMD_VERDICT_FRAG_SEQ;
  else if( sz < FRAG_HDR || sz > frag_max || at + sz > data_sz ) st = FD_AMD_VERDICT_FRAG_BAD;
  u32 const msz = st ? 0u : sz - FRAG_HDR;
  u64 const pub = st ? idle : chunk0 + at, sig = pub + 32UL, msg = msz ? pub + FRAG_HDR : idle;
  uint4 * const o = (uint4 *)(rec + i);
  o[0] = make_uint4( (u32)pub, (u32)(pub >> 32), (u32)sig, (u32)(sig >> 32) );
  o[1] = make_uint4( (u32)msg, (u32)(msg >> 32), msz, i * stride );   /* n * stride <= blob_max < 2^32: the callers' check */
  status[i] = (i8)st;
}

__global__ void __launch_bounds__(64)
k_frag_check( u32 n, u8 const * mcache, u64 mask, u64 seq0, i8 * status ) {
  u32 const i = blockIdx.x * 64u + threadIdx.x;
  if( i >= n || status[i] ) return;
  u64 const seq = seq0 + (u64)i;
  if( frag_ld_seq( mcache + ((seq & mask) << 5) ) != seq ) status[i] = (i8)FD_AMD_VERDICT_FRAG_SEQ;
}

__global__ void __launch_bounds__(64)
k_frag_verdict( u32 n, i8 * status, u8 const * mcache /* NULL: no recheck */, u64 mask, u64 seq0, i8 * d_err,
                i8 * m_err /* NULL: none */, u64 * tag ) {
  u32 const i = blockIdx.x * 64u + threadIdx.x;
  if( i >= n ) return;
  i8 st = status[i];
  if( mcache && !st ) {
    u64 const seq = seq0 + (u64)i;
    if( frag_ld_seq( mcache + ((seq & mask) << 5) ) != seq ) { st = (i8)FD_AMD_VERDICT_FRAG_SEQ; status[i] = st; }
  }
  if( !st || d_err[i] == (i8)FD_AMD_VERDICT_DEVICE ) return;
  d_err[i] = st;
  if( m_err ) m_err[i] = st;
  tag[i] = 0UL;
}

#endif
