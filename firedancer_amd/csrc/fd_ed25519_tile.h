/* firedancer_amd/csrc/fd_ed25519_tile.h
 *
 * The streaming tile's persistent kernel (scout, gather, transaction
 * layout, tile_chunk, k_tile_persist and its strict instantiation
 * k_tile_persist_strict), k_tile_synth and their two launch functions.  It
 * runs the bodies of the front and of all three DSM headers, and in strict
 * mode fd_ed25519_strict.h's decision; only fd_ed25519_kernels.hip includes
 * it.
 */

#ifndef FD_ED25519_TILE_H
#define FD_ED25519_TILE_H

#include "fd_ed25519_front.h"
#include "fd_ed25519_dsm.h"
#include "fd_ed25519_dsm4.h"
#include "fd_ed25519_dsm8.h"
#include "fd_txn_dev.h"
#include "fd_ed25519_strict.h"

/* ------------------------------------------------------------------ */
/* k_tile_persist: the streaming tile's persistent consumer.
 *
 * The reference verify tile (src/app/frank/load/fd_frank_verify_synth_load.c:
 * 219-437) verifies one frag per call on one core; N tiles scale it.  Here
 * one launch per tile run holds every wave slot of the GPU (one single-wave
 * workgroup per slot) and verifies what the tile's host thread hands over
 * through mapped host memory: the frags' ring entries, and CHUNK
 * descriptors {first ring index, count, mode} that the host cuts from each
 * hand-off (mode: 8 lanes per signature while the GPU is lightly loaded,
 * for latency; 1 lane per signature under load, for throughput).
 *
 *   wave 0 (scout)   the only poller of host memory: it mirrors the host's
 *                    descriptor head, its stop request and a heartbeat into
 *                    one word per XCD (device memory, one line each);
 *   waves 1..        take a TICKET (one atomic add per chunk, never
 *                    retried), wait on their XCD's mirror word until
 *                    descriptor `ticket` exists, read it, and verify the
 *                    chunk alone: copy the frags in (and, zero-copy, out to
 *                    their output frames), k_prep's body, k_decomp's body,
 *                    then k_dsm8's body or k_dsm's body, then verdict + tag
 *                    to the mapped result ring, released after a
 *                    system-scope fence so the host sees them in full.
 *
 * Contention is what this layout avoids: a first version let every idle
 * wave load the shared head and CAS a claim counter; 2000 waves on one
 * line made every atomic take ~20 us and stalled the CUs' memory pipelines
 * (every phase, the DSM loop included, ran 8-10x slow).  Now each chunk
 * costs one atomic add, and a waiting wave polls its XCD's mirror with a
 * back-off proportional to how far its ticket is from the head.  Every
 * spin is bounded: the scout flags an error after `watchdog` ticks without
 * a host heartbeat, a waiting wave exits after `watchdog` ticks with an
 * unchanged mirror word, so the grid always drains.
 *
 * Same bodies as the batch kernels, same workspace layout (one N = 64
 * workspace per wave): identical limbs and verdicts. */

#define TILE_FRAME (1408u)   /* FD_VERIFY_AMD_FRAME_SZ */
#define TILE_MODE_THR   (0u)   /* 1 lane per signature, <= 64 slots (k_dsm's body) */
#define TILE_MODE_LAT8  (1u)   /* 8 lanes per signature, <= 8 slots (k_dsm8's body) */
#define TILE_MODE_QUAD4 (2u)   /* 4 lanes per signature, <= 16 slots (k_dsm4's body) */

__device__ __forceinline__ u64 ld_sys64( u64 const * p ) { return __hip_atomic_load( (u64 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM ); }
__device__ __forceinline__ u32 ld_sys32( u32 const * p ) { return __hip_atomic_load( (u32 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM ); }
__device__ __forceinline__ void st_sys64( u64 * p, u64 v ) { __hip_atomic_store( p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM ); }
__device__ __forceinline__ void st_sys32( u32 * p, u32 v ) { __hip_atomic_store( p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM ); }
__device__ __forceinline__ u64 ld_dev64( u64 const * p ) { return __hip_atomic_load( (u64 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT ); }
__device__ __forceinline__ u32 ld_dev32( u32 const * p ) { return __hip_atomic_load( (u32 *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT ); }
__device__ __forceinline__ void st_dev32( u32 * p, u32 v ) { __hip_atomic_store( p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT ); }
__device__ __forceinline__ void st_dev64( u64 * p, u64 v ) { __hip_atomic_store( p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT ); }
__device__ __forceinline__ u64 rfl64( u64 v ) {
  return ((u64)(u32)__builtin_amdgcn_readfirstlane( (int)(u32)(v >> 32) ) << 32) | (u32)__builtin_amdgcn_readfirstlane( (int)(u32)v );
}

/* mirror word: descriptor head | scout heartbeat << 48 | err << 62 | stop << 63 */
#define TILE_MW_HEAD(w)  ((w) & ((1UL << 48) - 1UL))
#define TILE_MW_ERR      (1UL << 62)
#define TILE_MW_STOP     (1UL << 63)

/* per-wave scratch: an N = 64 workspace, then the chunk's frames and planes */
struct tile_scratch_t { size_t mir, pub, sig, off, sz, err, skp, tx, total; };
__host__ __device__ constexpr tile_scratch_t tile_scratch_layout( void ) {
  tile_scratch_t S = {}; size_t o = ws_al( ws_layout_const( 64 ).total );
  S.mir = o; o = ws_al( o + 64UL*TILE_FRAME );
  S.pub = o; o = ws_al( o + 64UL*32UL );
  S.sig = o; o = ws_al( o + 64UL*64UL );
  S.off = o; o = ws_al( o + 64UL*4UL );
  S.sz  = o; o = ws_al( o + 64UL*4UL );
  S.err = o; o = ws_al( o + 64UL );
  S.skp = o; o = ws_al( o + 64UL );          /* TXN: per slot, nonzero = its transaction failed to parse */
  S.tx  = o; o = ws_al( o + 64UL*4UL );      /* TXN: per entry, first slot | slots << 8 | parsed << 31 */
  S.total = o;
  return S;
}

size_t fd_amd_tile_scratch_stride( void ) { return tile_scratch_layout().total; }

/* The scout (wave 0, lane 0): host words -> the XCDs' mirror words, and
   back to the host every ~10 us its clock (the host maps the waves' time
   stamps onto its own clock with it; its first store tells the host the
   kernel started) and the count of finished chunks (the host's progress
   watchdog). */
__device__ __forceinline__ void
tile_scout( fd_amd_tile_dctl_t * D, fd_amd_tile_hctl_t * H, u64 watchdog ) {
  __builtin_amdgcn_s_setprio( 3 );   /* beside the workers' aged chunks on its SIMD */
  u64 word = ld_dev64( &D->mw[0].w ), lastb = ~0UL, beat = 0UL;
  u64 tb = __builtin_amdgcn_s_memrealtime(), tpub = tb, tclk = tb;
  st_sys64( &H->gclock, tb );
  for( ;; ) {
    u64 h = ld_sys64( &H->head ), b = ld_sys64( &H->beat );
    u32 st = ld_sys32( &H->stop );
    u64 now = __builtin_amdgcn_s_memrealtime();
    if( now - tclk >= 1000UL ) {
      tclk = now;
      st_sys64( &H->gdone, ld_dev64( &D->done ) );
      st_sys64( &H->gclock, now );
    }
    if( b != lastb ) { lastb = b; tb = now; }
    bool dead = now - tb > watchdog;
    if( dead ) st_sys32( &H->kerr, 1u );
    /* the heartbeat field advances at most every 10 us (it only keeps the
       waiting waves' own watchdog quiet) */
    if( now - tpub > 1000UL && now - tb < 1000UL ) { beat++; tpub = now; }
    u64 w = (h & ((1UL << 48) - 1UL)) | ((beat & 0x3fffUL) << 48) | (dead ? TILE_MW_ERR : 0UL) | (st ? TILE_MW_STOP : 0UL);
    if( w != word ) {
      word = w;
      _Pragma("unroll") for( int x=0; x<FD_AMD_TILE_MIRRORS; x++ ) st_dev64( &D->mw[x].w, w );
    }
    if( st || dead ) break;
    __builtin_amdgcn_s_sleep( 2 );
  }
}

/* nw little-endian words from an unaligned address inside a frame: nw + 1
   aligned dword loads funnel-shifted by the misalignment (the frame has
   room for the extra word: frames are FD_VERIFY_AMD_FRAME_SZ >= MTU + 4). */
template<int NW>
__device__ __forceinline__ void
ld_words_unaligned( u8 const * p, u32 (&o)[NW] ) {
  u32 const * a = (u32 const *)((size_t)p & ~(size_t)3);
  u32 const sh = (u32)(size_t)p & 3u;
  u32 w[NW + 1];
  _Pragma("unroll") for( int k=0; k<=NW; k++ ) w[k] = a[k];
  _Pragma("unroll") for( int k=0; k<NW; k++ ) o[k] = __builtin_amdgcn_alignbyte( w[k+1], w[k], sh );   /* byte shift */
}

/* TXN framing: the chunk's k ring entries are wire transactions (frames
   0..k-1 of mir) carrying e_k signature slots each (the host's count,
   fd_amd_txn_slots1; the chunk's total <= 64).  Lane q < k parses
   transaction q (fd_txn_parse semantics, fd_txn_dev.h); lane s < n then
   lays slot s out for the verify bodies: signature i of its transaction
   with account address i over the shared message bytes in mir
   (fd_txn.h:159-217), or skip = FD_TXN_AMD_ERR_PARSE when the transaction
   failed to parse (or parsed to a signature count other than the host's:
   fail closed).  tx[q] keeps the entry's first slot, slot count and parse
   flag for the per-transaction reduce.  lds: >= 64 x 5 words of scratch
   LDS (the DSM bodies' event rows, unused until then).  Returns n, the
   chunk's signature slots (wave-uniform). */
__device__ __forceinline__ u32
tile_txn_layout( u32 l, u32 k, u32 e_sz, u32 e_k, u8 const * __restrict__ mir, u8 * __restrict__ pub,
                 u8 * __restrict__ sig, u32 * __restrict__ off, u32 * __restrict__ sz, i8 * __restrict__ skp,
                 u32 * __restrict__ tx, u32 * __restrict__ lds ) {
  u32 const kk = l < k ? e_k : 0u;
  u32 inc = kk;
  _Pragma("unroll") for( int d=1; d<64; d<<=1 ) {
    u32 const o = (u32)__shfl_up( (int)inc, (unsigned)d );
    if( l >= (u32)d ) inc += o;
  }
  u32 const base = inc - kk;
  u32 const n = min( (u32)__shfl( (int)inc, 63 ), 64u );
  u32 * own  = lds;            /* [64]: slot -> entry */
  u32 * info = lds + 64;       /* [64][5]: sig_off, acct_off, msg_off (~0: not parsed), frag size, first slot */
  if( l < k ) {
    u32 nsig = 0u, sig_off = 0u, acct_off = 0u, msg_off = 0u;
    u32 const fp = fd_txn_dev::txn_parse( mir + (size_t)l * TILE_FRAME, e_sz, (u8 *)0, 0u, &nsig, &sig_off, &acct_off, &msg_off );
    u32 const ok = fp != 0u && nsig == kk && base + kk <= 64u;   /* the host packs <= 64 slots per chunk */
    for( u32 i=0u; i<kk && base + i < 64u; i++ ) own[base + i] = l;
    u32 * in = info + 5u*l;
    in[0] = sig_off; in[1] = acct_off; in[2] = ok ? msg_off : 0xFFFFFFFFu; in[3] = e_sz; in[4] = base;
    tx[l] = base | (kk << 8) | (ok << 31);
  }
  __syncthreads();
  if( l < n ) {
    u32 const q = own[l];
    u32 const * in = info + 5u*q;
    u32 const i = l - in[4];
    u32 const msg_off = in[2];
    if( msg_off != 0xFFFFFFFFu ) {
      u8 const * f = mir + (size_t)q * TILE_FRAME;
      u32 a[8], g[16];
      ld_words_unaligned<8>( f + in[1] + 32u*i, a );
      ld_words_unaligned<16>( f + in[0] + 64u*i, g );
      uint4 * P = (uint4 *)(pub + 32u*l);
      uint4 * G = (uint4 *)(sig + 64u*l);
      P[0] = make_uint4( a[0], a[1], a[2], a[3] );   P[1] = make_uint4( a[4], a[5], a[6], a[7] );
      G[0] = make_uint4( g[0], g[1], g[2], g[3] );   G[1] = make_uint4( g[4], g[5], g[6], g[7] );
      G[2] = make_uint4( g[8], g[9], g[10], g[11] ); G[3] = make_uint4( g[12], g[13], g[14], g[15] );
      off[l] = q * TILE_FRAME + msg_off; sz[l] = in[3] - msg_off; skp[l] = 0;
    } else {
      off[l] = 0u; sz[l] = 0u; skp[l] = (i8)TXN_ERR_PARSE;
    }
  }
  return n;
}

/* Copy a chunk's k frags in: frame q (16-B word w of it) by lane 16 (q % 4)
   + (w % 16) of round q / 4; four rounds (16 frames) have every load
   issued before any store, so a 64-frag chunk waits four round trips to
   the frames' memory (host memory over PCIe in zero-copy mode), not
   sixteen (gather 92 -> 62 us per chunk at saturation, paced service p50
   1.30 -> 1.25 ms: profiles/r05_tile_pool_experiment.txt).  Frames are
   <= 1328 B = 83 words, chunk-aligned (every 16-B word whole): up to six
   words per lane per round.  Zero copy: every word also goes out to the
   frag's output frame; PUB_SIG_MSG: pub and sig to their planes. */
__device__ __forceinline__ void
tile_gather( fd_amd_tile_args_t const & A, u32 k, u32 l, u32 e_src, u32 e_out, u32 e_sz, u8 * __restrict__ mir,
             u8 * __restrict__ pub, u8 * __restrict__ sig, bool txn ) {
  u32 const g = l >> 4, j = l & 15u;
  for( u32 q0 = 0; q0 < k; q0 += 16u ) {
    uint4 v[4][6];
    u32 nv[4];
    _Pragma("unroll") for( int h=0; h<4; h++ ) {
      u32 const q = q0 + 4u*(u32)h + g;
      u32 const src = (u32)__shfl( (int)e_src, (int)(q & 63u) );
      u32 const fs  = (u32)__shfl( (int)e_sz,  (int)(q & 63u) );
      nv[h] = q < k ? (fs + 15u) >> 4 : 0u;
      uint4 const * s = (uint4 const *)(A.src + ((size_t)src << 6));
      _Pragma("unroll") for( int r=0; r<6; r++ ) {
        u32 w = j + 16u*(u32)r;
        v[h][r] = w < nv[h] ? s[w] : make_uint4( 0u, 0u, 0u, 0u );
      }
    }
    _Pragma("unroll") for( int h=0; h<4; h++ ) {
      u32 const q = q0 + 4u*(u32)h + g;
      u32 const oc = (u32)__shfl( (int)e_out, (int)(q & 63u) );
      uint4 * m = (uint4 *)(mir + (size_t)(q & 63u) * TILE_FRAME);
      uint4 * o = A.out ? (uint4 *)(A.out + ((size_t)oc << 6)) : (uint4 *)0;
      _Pragma("unroll") for( int r=0; r<6; r++ ) {
        u32 w = j + 16u*(u32)r;
        if( w < nv[h] ) { m[w] = v[h][r]; if( o ) o[w] = v[h][r]; }
      }
      if( q < k && !txn ) {
        if( j < 2u )      ((uint4 *)(pub + 32u*q))[j]      = v[h][0];
        else if( j < 6u ) ((uint4 *)(sig + 64u*q))[j - 2u] = v[h][0];
      }
    }
  }
}

/* Verify ring entries [c0, c0 + k) (k <= 64) on this wave, claimed at
   s_memrealtime tc, in chunk mode `mode` (TILE_MODE_*: 1 lane per signature,
   8 lanes (k_dsm8's body) or 4 lanes (k_dsm4's body); the host keeps a
   chunk's slots within the mode's 64 / 8 / 16 lanes).  PUB_SIG_MSG: entry q is signature slot q.  TXN
   (A.txn): entry q is a wire transaction whose slots tile_txn_layout lays
   out, and its result is the transaction's verdict.  STRICT: the strict
   RFC 8032 verdicts (k_strict's rule, fd_ed25519_strict.h) instead of the
   reference's; tile_chunk<false> holds no trace of that step. */
template<bool STRICT>
__device__ __forceinline__ void
tile_chunk(fd_amd_tile_args_t const & A, u64 c0, u32 k, u32 mode, u8 * __restrict__ scr, ws_layout_t L,
            tile_scratch_t const & S, i32 (* __restrict__ bi)[48], u64 (* __restrict__ evl)[33], u64 * pt, u64 tc,
            u32 pp = 0u ) {
  /* pp = pair | pair_seq << 2 (quad pairs, FD_AMD_TILE_PAIR); pair: 0 none;
     1 sub 0 -- the front of all k entries, then the pair's flag =
     pair_seq + 1, then entries [0, 16); 2 sub 1 (the caller saw that flag)
     -- entries [16, k) on sub 0's front */
  u32 const pair = pp & 3u;
  /* pt (A.prof, set by the diagnostics build's host only): s_memrealtime
     ticks spent in gather [0], prep [6], decomp [1], DSM [2], results [3];
     wave-uniform */
  u64 ts = A.prof ? __builtin_amdgcn_s_memrealtime() : 0UL;
# define TILE_STAMP( k_ ) do { if( A.prof ) { u64 t_ = __builtin_amdgcn_s_memrealtime(); if( !threadIdx.x ) pt[k_] += t_ - ts; ts = t_; } } while(0)
  /* opaque per chunk: otherwise the compiler hoists every per-lane address
     of the bodies out of the persistent loop and spills them */
  {
    __attribute__((address_space(1))) u8 * g = (__attribute__((address_space(1))) u8 *)scr;
    asm volatile( "" : "+s"(g) );
    scr = (u8 *)g;     /* still known global: global, not flat, accesses */
  }
  u32 l = threadIdx.x;
  asm volatile( "" : "+v"(l) );
  u8 * ws = scr; u8 * mir = scr + S.mir; u8 * pub = scr + S.pub; u8 * sig = scr + S.sig;
  u32 * off = (u32 *)(scr + S.off); u32 * sz = (u32 *)(scr + S.sz); i8 * err = (i8 *)(scr + S.err);

  /* 1. the chunk's ring entries, lane q holds entry q (host memory: system-scope loads) */
  bool const txn = A.txn != 0u;
  /* a pair's sub 1 runs the front on no entries (its barriers only: a
     branch round the front costs the loop a VGPR spill) */
  u32 const kf = pair == 2u ? 0u : k;
  u32 e_src = 0u, e_out = 0u, e_sz = 96u, e_k = 0u;
  if( l < kf ) {
    u64 const * ep = (u64 const *)(A.ent + ((c0 + l) & A.mask));
    u64 w0 = ld_sys64( ep ), w1 = ld_sys64( ep + 1 );
    e_src = (u32)w0; e_out = (u32)(w0 >> 32); e_sz = (u32)w1; e_k = (u32)(w1 >> 32);
  }
  /* 2. copy the frags in (tile_gather) */
  tile_gather( A, kf, l, e_src, e_out, e_sz, mir, pub, sig, txn );
  if( l < kf && !txn ) { off[l] = l * TILE_FRAME + 96u; sz[l] = e_sz - 96u; }
  __syncthreads();
  /* TXN: parse and lay the chunk's signature slots out (n of them) */
  i8 * skp = (i8 *)(scr + S.skp);
  u32 * tx = (u32 *)(scr + S.tx);
  u32 const n = txn ? tile_txn_layout( l, k, e_sz, e_k, mir, pub, sig, off, sz, skp, tx, (u32 *)&evl[0][0] ) : kf;
  if( txn ) __syncthreads();
  TILE_STAMP( 0 );
  /* 3. the verify pipeline on the chunk (k_prep, k_decomp, k_dsm / k_dsm8 / k_dsm4 bodies) */
  prep_body( l, n, pub, sig, off, sz, mir, err, ws, L, txn ? (i8 const *)skp : (i8 const *)0 );
  __syncthreads();
  TILE_STAMP( 6 );
  decomp_body( l, n, pub, sig, err, ws, L, true );                 /* points 0..63: signatures 0..31 */
  if( n > 32u ) decomp_body( l + 64u, n, pub, sig, err, ws, L, true );
  __syncthreads();
  TILE_STAMP( 1 );
  if( pair == 1u ) {
    /* the pair's front is done: every lane's workspace writes out of this
       XCD's L2 (agent-scope release), then the flag sub 1 waits on */
    __builtin_amdgcn_fence( __ATOMIC_RELEASE, "agent" );
    __syncthreads();
    if( l == 0u ) st_dev32( A.pair_flag + ((pp >> 2) & A.pair_mask), (pp >> 2) + 1u );
  }
  /* this wave's signatures: all k, or a pair sub's 16 */
  u32 const g0 = pair == 2u ? 64u : 0u;                 /* k_dsm4's lane index: signature (g0 + l) >> 2 */
  u32 const nd = pair == 1u ? min( k, 16u ) : pair == 2u ? k : n;
  if( mode == TILE_MODE_LAT8 )       dsm8_body( l, n, err, ws, L, 0, bi, evl, tc );
  else if( mode == TILE_MODE_QUAD4 ) dsm4_body( g0 + l, nd, err, ws, L, 0, bi, evl, tc );
  else                               dsm_lane_body( l, n, err, ws, L, 0, bi, evl, tc );
  __builtin_amdgcn_s_setprio( 0 );
  __syncthreads();
  if constexpr( STRICT ) {
    /* the strict overlay, one lane per signature slot, over the slots whose
       DSM this wave ran (a pair's sub 1: [16, k) = dsm4_body's g0 >> 2 on),
       from the parked layout of the chunk's mode.  strict_decide's invariant
       holds as in k_strict: prep_body, decomp_body and the DSM body above
       are the batch kernels' bodies.  A slot whose transaction failed to
       parse keeps its skip.  No wait and no loop over memory: the chunk's
       own scratch, written before the barrier above.  Every lane reaches
       the barrier below; the result stores then read err[] as ever. */
    u32 const si = (g0 >> 2) + l;
    if( si < nd && !(txn && skp[si]) ) {
      int const kind = mode == TILE_MODE_LAT8 ? STRICT_DSM8 : mode == TILE_MODE_QUAD4 ? STRICT_DSM4 : STRICT_DSM;
      err[si] = (i8)strict_decide( si, pub, sig, (int)err[si], ws, L, kind );
    }
    __syncthreads();
  }
  TILE_STAMP( 2 );
  /* 4. results: tags (and, zero-copy, the output frames above) first, one
        system-scope release, then the words the host polls.  TXN: an entry's
        verdict is its parse failure, else the first failing signature's
        code in signature order, else 0 (k_txn_reduce); its tag is its first
        signature's */
  u32 const e0 = pair == 2u ? 16u : 0u, e1 = pair == 1u ? min( k, 16u ) : k;   /* this wave's entries */
  u32 const q = e0 + l;
  u64 const idx = c0 + q, j = idx & A.mask;
  u64 tag = 0UL; i8 v = 0;
  if( q < e1 ) {
    if( !txn ) { tag = ((u64 const *)(ws + L.tag))[q]; v = err[q]; }
    else {
      u32 const w = tx[l], b = w & 0xffu, kk = (w >> 8) & 0xffu;
      if( !(w >> 31) ) v = (i8)TXN_ERR_PARSE;
      else for( u32 i=0u; i<kk; i++ ) { i8 const e = err[b + i]; if( e ) { v = e; break; } }
      if( kk ) tag = ((u64 const *)(ws + L.tag))[b];
    }
    st_sys64( A.res_tag + j, tag );
  }
  if( A.res_time && q < e1 ) st_sys64( A.res_time + j, (u64)(u32)tc | ((u64)(u32)__builtin_amdgcn_s_memrealtime() << 32) );
  __builtin_amdgcn_fence( __ATOMIC_RELEASE, "" );
  asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
  u64 const wd = ((idx + 1UL) << 8) | (u64)(u8)v;
  if( q < e1 ) st_sys64( A.res_word + j, wd );
  TILE_STAMP( 3 );
# undef TILE_STAMP
}

/* The persistent kernel's text, once per verdict mode: NAME_ runs
   tile_chunk<STRICT_>.  A macro and not a shared inline body: with the loop
   in a forceinline template called by two thin kernels the reference
   kernel's code changed (3 more SGPR spills, 60 more instructions), while
   two expansions of the same text leave k_tile_persist's instructions as
   they were before the strict kernel existed. */
#define TILE_PERSIST_KERNEL( NAME_, STRICT_ )                                                                                            \
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2)))                                                            \
NAME_( fd_amd_tile_args_t A ) {                                                                                                          \
  constexpr ws_layout_t    L = ws_layout_const( 64 );   /* every plane offset an immediate */                                            \
  constexpr tile_scratch_t S = tile_scratch_layout();                                                                                    \
  __shared__ __attribute__((aligned(16))) i32 bi[8][48];                                                                                 \
  __shared__ u64 evl[64][33];                                                                                                            \
  fd_amd_tile_dctl_t * D = A.dctl;                                                                                                       \
  u32 const l = threadIdx.x;                                                                                                             \
  if( blockIdx.x == 0u ) {                                                                                                               \
    if( l == 0u ) tile_scout( D, A.hctl, A.watchdog );                                                                                   \
    return;                                                                                                                              \
  }                                                                                                                                      \
  bi12_fill( bi );                                                                                                                       \
  __syncthreads();                                                                                                                       \
  /* this wave's mirror word: its XCD's (HW_REG_XCC_ID) */                                                                               \
  u32 const xcc = __builtin_amdgcn_s_getreg( 20 | (0 << 6) | (3 << 11) ) % FD_AMD_TILE_MIRRORS;                                          \
  u64 const * mw = &D->mw[xcc].w;                                                                                                        \
  u8 * scr = A.scratch + (size_t)blockIdx.x * S.total;                                                                                   \
  /* per-wave tallies in LDS, not registers (the DSM bodies want every VGPR):                                                            \
     [0..7] diagnostics build (A.prof) gather, front, DSM, results, wait,                                                                \
     fence, -, -; [8..13] dctl->stat: latency chunks, throughput chunks,                                                                 \
     their frags, quad chunks, their frags */                                                                                            \
  __shared__ u64 s_tally[16];                                                                                                            \
  if( l < 16u ) s_tally[l] = 0UL;                                                                                                        \
  u64 * const pt = s_tally;                                                                                                              \
  /* A run-time flag (the host sets it only in the diagnostics build), not a                                                             \
     compile-time constant: with the profiling branches folded away the                                                                  \
     compiler gives this kernel all 256 VGPRs, and at 256 its scout wave                                                                 \
     stopped ~0.7 ms into every run, called or inlined (profiles/                                                                        \
     r04_tile_scout_vgpr_ab.txt, r05_scout_stop_cause.txt); build.py refuses                                                             \
     a build at 256. */                                                                                                                  \
  bool const prof = A.prof != 0u;                                                                                                        \
  for( ;; ) {                                                                                                                            \
    u64 t = 0;                                                                                                                           \
    if( l == 0u ) t = atomicAdd( (unsigned long long *)&D->ticket, 1ULL );                                                               \
    t = rfl64( t );                                                                                                                      \
    /* wait for descriptor t: poll the mirror, backing off with the                                                                      \
       distance to the head (the next in line polls every ~0.2 us) */                                                                    \
    u64 t0 = __builtin_amdgcn_s_memrealtime(), tw = t0, last = ~0UL;                                                                     \
    bool go = false;                                                                                                                     \
    for( ;; ) {                                                                                                                          \
      u64 const w = rfl64( l == 0u ? ld_dev64( mw ) : 0UL );                                                                             \
      if( TILE_MW_HEAD( w ) > t ) { go = true; break; }                                                                                  \
      if( w & (TILE_MW_ERR | TILE_MW_STOP) ) break;                                                                                      \
      u64 const now = __builtin_amdgcn_s_memrealtime();                                                                                  \
      if( w != last ) { last = w; tw = now; }                                                                                            \
      else if( now - tw > A.watchdog ) break;       /* no scout (or host) for that long: give up */                                      \
      u64 const d = t - TILE_MW_HEAD( w );                                                                                               \
      u32 const nap = d < 2UL ? 1u : d < 64UL ? (u32)d : 64u;                                                                            \
      for( u32 z = 0; z < nap; z++ ) __builtin_amdgcn_s_sleep( 4 );                                                                      \
    }                                                                                                                                    \
    if( prof && !l ) pt[4] += __builtin_amdgcn_s_memrealtime() - t0;                                                                     \
    if( !go ) break;                                                                                                                     \
    u64 const tc = __builtin_amdgcn_s_memrealtime();   /* claimed */                                                                     \
    /* descriptor t (host memory): { first ring index, count | FD_AMD_TILE_LAT | FD_AMD_TILE_QUAD } */                                   \
    u64 c = 0, cm = 0;                                                                                                                   \
    if( l == 0u ) {                                                                                                                      \
      u64 const * dp = (u64 const *)(A.desc + (t & A.mask));                                                                             \
      c = ld_sys64( dp ); cm = ld_sys64( dp + 1 );                                                                                       \
    }                                                                                                                                    \
    c = rfl64( c ); cm = rfl64( cm );                                                                                                    \
    u32 const take = FD_AMD_TILE_COUNT( (u32)cm );                                                                                       \
    u32 const md = ((u32)cm & FD_AMD_TILE_LAT) ? TILE_MODE_LAT8 : ((u32)cm & FD_AMD_TILE_QUAD) ? TILE_MODE_QUAD4 : TILE_MODE_THR;        \
    /* quad pair: its shared workspace and flag; sub 1 first waits for sub 0's front */                                                  \
    u32 const pr = ((u32)cm & FD_AMD_TILE_PAIR) && A.pair_ws && !A.txn && md == TILE_MODE_QUAD4 ? 1u + (u32)((cm >> 32) & 1UL) : 0u;     \
    u32 const pseq = (u32)(cm >> 33) & 0x3fffffffu;                                                                                      \
    u8 * cscr = pr ? A.pair_ws + (size_t)(pseq & A.pair_mask) * S.total : scr;                                                           \
    u32 * pf = pr ? A.pair_flag + (pseq & A.pair_mask) : (u32 *)0;                                                                       \
    bool pok = true;                                                                                                                     \
    if( pr == 2u ) {                                                                                                                     \
      u64 const tp = __builtin_amdgcn_s_memrealtime();                                                                                   \
      for( ;; ) {                                                                                                                        \
        u32 const f = (u32)__builtin_amdgcn_readfirstlane( (int)(l == 0u ? ld_dev32( pf ) : 0u) );                                       \
        if( f == pseq + 1u ) break;                                                                                                      \
        u64 const w = rfl64( l == 0u ? ld_dev64( mw ) : 0UL );                                                                           \
        if( (w & TILE_MW_ERR) || __builtin_amdgcn_s_memrealtime() - tp > A.watchdog ) { pok = false; break; }                            \
        __builtin_amdgcn_s_sleep( 2 );                                                                                                   \
      }                                                                                                                                  \
      __builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "agent" );   /* sub 0's workspace writes (another XCD's L2) */                           \
    }                                                                                                                                    \
    /* the frames were written by the host (copy mode) or the producer                                                                   \
       (zero-copy) into host memory: drop this CU's stale lines first */                                                                 \
    u64 const tf = prof ? __builtin_amdgcn_s_memrealtime() : 0UL;                                                                        \
    __builtin_amdgcn_fence( __ATOMIC_ACQUIRE, "" );                                                                                      \
    asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );                                                                                   \
    if( prof && !l ) pt[5] += __builtin_amdgcn_s_memrealtime() - tf;                                                                     \
    if( take && take <= 64u && pok && (!pr || (take > 16u && take <= 32u)) )                                                             \
      tile_chunk<STRICT_>( A, c, take, md, cscr, L, S, bi, evl, pt, tc, pr | pseq << 2 );                                                \
    if( !l ) {                                                                                                                           \
      /* dctl->stat slots: chunks, frags -- latency 0, 2; throughput 1, 3; quad 4, 5 (a pair sub is a quad chunk) */                     \
      u32 const tc_ = md == TILE_MODE_LAT8 ? 0u : md == TILE_MODE_THR ? 1u : 4u;                                                         \
      u32 const tf_ = md == TILE_MODE_LAT8 ? 2u : md == TILE_MODE_THR ? 3u : 5u;                                                         \
      s_tally[8u + tc_] += 1UL; s_tally[8u + tf_] += pr == 1u ? 16u : pr == 2u ? take - 16u : take;                                      \
      atomicAdd( (unsigned long long *)&D->done, 1ULL );   /* progress, mirrored to the host by the scout */                             \
    }                                                                                                                                    \
  }                                                                                                                                      \
  if( l == 0u ) {                                                                                                                        \
    _Pragma("unroll") for( int q=0; q<6; q++ ) atomicAdd( (unsigned long long *)&D->stat[q], (unsigned long long)s_tally[8 + q] );       \
    if( prof ) { _Pragma("unroll") for( int q=0; q<8; q++ ) atomicAdd( (unsigned long long *)&D->prof[q], (unsigned long long)pt[q] ); } \
  }                                                                                                                                      \
}

TILE_PERSIST_KERNEL( k_tile_persist, false )          /* FD_ED25519_AMD_MODE_REFERENCE */
TILE_PERSIST_KERNEL( k_tile_persist_strict, true )    /* FD_ED25519_AMD_MODE_STRICT: the same loop, strict overlay per chunk */

#ifdef FD_AMD_DIAG
/* Diagnostics build only.  Measurement aid: k_tile_persist's chunk pipeline without the host
   hand-off (no tickets, no polling, nothing in mapped memory): wave w runs
   `iters` chunks of k ring entries, [(w iters + it) k, +k), with every
   argument in device memory (fd_amd_tile_synth, tools/tile_synth.py). */
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2)))
k_tile_synth( fd_amd_tile_args_t A, u32 iters, u32 eight ) {
  constexpr ws_layout_t    L = ws_layout_const( 64 );
  constexpr tile_scratch_t S = tile_scratch_layout();
  __shared__ __attribute__((aligned(16))) i32 bi[8][48];
  __shared__ u64 evl[64][33];
  bi12_fill( bi );
  __syncthreads();
  __shared__ u64 pt[8];
  if( threadIdx.x < 8u ) pt[threadIdx.x] = 0UL;
  __syncthreads();
  u32 const md = eight == 1u ? TILE_MODE_LAT8 : eight == 2u ? TILE_MODE_QUAD4 : TILE_MODE_THR;   /* eight: 0 / 1 / 2 */
  u32 const k = md == TILE_MODE_LAT8 ? 8u : md == TILE_MODE_QUAD4 ? 16u : 64u;
  if( A.hctl && blockIdx.x == gridDim.x - 1u ) {
    /* A/B: a scout-like wave polling the host control words until the
       others are done (bounded by the watchdog) */
    if( threadIdx.x == 0u ) {
      u64 const t0 = __builtin_amdgcn_s_memrealtime();
      u64 acc = 0;
      while( __hip_atomic_load( (u64 *)&A.dctl->stat[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT ) < (u64)(gridDim.x - 1u) &&
             __builtin_amdgcn_s_memrealtime() - t0 < A.watchdog ) {
        acc += ld_sys64( &A.hctl->head ) + ld_sys64( &A.hctl->beat ) + ld_sys32( &A.hctl->stop );
        __builtin_amdgcn_s_sleep( 2 );
      }
      A.dctl->stat[1] = acc;
    }
    return;
  }
  u8 * scr = A.scratch + (size_t)blockIdx.x * S.total;
  for( u32 it = 0; it < iters; it++ )
    tile_chunk<false>( A, ((u64)blockIdx.x * iters + it) * k, k, md, scr, L, S, bi, evl, pt, 0UL );
  if( A.prof && threadIdx.x == 0u ) {
    _Pragma("unroll") for( int q=0; q<8; q++ ) atomicAdd( (unsigned long long *)&A.dctl->prof[q], (unsigned long long)pt[q] );
  }
  if( A.hctl && threadIdx.x == 0u ) atomicAdd( (unsigned long long *)&A.dctl->stat[0], 1ULL );
}

int
fd_amd_launch_tile_synth( fd_amd_tile_args_t const * a, uint32_t waves, uint32_t iters, int eight, hipStream_t stream ) {
  if( !waves || !iters ) return -1;
  hipLaunchKernelGGL( k_tile_synth, dim3(waves), dim3(64), 0, stream, *a, iters, (u32)eight );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#endif /* FD_AMD_DIAG */

/* strict: nonzero launches k_tile_persist_strict (the run's verdict mode is
   the choice of kernel, not a field k_tile_persist would read) */
int
fd_amd_launch_tile_persist( fd_amd_tile_args_t const * a, uint32_t waves, hipStream_t stream, int strict ) {
  if( waves < 2u ) return -1;
  (void)hipGetLastError();   /* the check below is the launch's own: every earlier call checked its return code */
  if( strict ) hipLaunchKernelGGL( k_tile_persist_strict, dim3(waves), dim3(64), 0, stream, *a );
  else         hipLaunchKernelGGL( k_tile_persist,        dim3(waves), dim3(64), 0, stream, *a );
  hipError_t const e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;   /* the HIP error, for the caller's message */
}

#endif /* FD_ED25519_TILE_H */
