/* firedancer_amd/csrc/fd_ed25519_emit.h -- the survivors' output frames
   (include/fd_ed25519_amd.h, "Output frames"): for survivor j of a
   submission, item i = keep[j], one frame at out + emit_off[j] of emit_sz[j]
   bytes,

     signature family    pub[i] (32) | sig[i] (64) | msg[i] (sz[i])
     transaction family  payload (P) | zeros up to P16 = round_up( P, 16 ) |
                         fd_txn_t (F, even) | P as a little-endian u16

   emit_off[0] = 0, emit_off[j+1] = emit_off[j] + round_up( emit_sz[j], 128 ).

   Two parts.  The first, fd_amd_emit_frame, is the size and stride
   arithmetic: ONE function that the host rule (fd_ed25519_host.cpp, plain
   C++) and the kernels below both compile, so the CPU tests exercise the
   arithmetic that computes device addresses.  The second, the kernels, is
   compiled only where fd_ed25519_gather.h was included first (the .hip unit).

   Kernels, ordered by the stream; no workgroup waits for another, no atomics,
   no spinning, vector stores only:

     k_emit_size_*  one lane per survivor: the item, emit_sz, the stride in
                    units of 128 B, and the totals of every 64 of those
     the scan       fd_amd_launch_bscan64: one workgroup loops over the totals
     k_emit_off     per 64-block: emit_off
     k_emit_sig /   the store: k_gather turned round, 16 lanes per frame
     k_emit_txn

   The store.  Sources have any byte alignment and are read under
   fd_ed25519_gather.h's ACCESS INVARIANT, with its gather_ld / gather_shift /
   gather_shfl: every load is a naturally aligned 16-B word that overlaps the
   range being copied; a lane takes the word after its own from the lane that
   loaded it; a lane with no word to fetch loads 16 B of the scratch instead.
   Every destination word is a 16-aligned 16-B store inside the frame's own
   stride: frames start on multiples of 128 from a 64-aligned base, the
   message starts at byte 96 of its frame and the descriptor at P16.  Bytes of
   a frame's last word behind the frame are stored as zeros (emit_keep_bytes),
   so a frame writes exactly [ emit_off, emit_off + round_up( emit_sz, 16 ) ).
   The one place where two pieces share a store is the transaction frame's
   last word: the descriptor's tail, then the u16.  Each 16-lane group has
   EMIT_G frames in flight and every load of a pass is issued before its first
   store.  A wave takes blocks of 4 EMIT_G frames gridDim.x apart, so the
   grid, not n, bounds the writes to host memory in flight.

   Capacity: frame j is stored only if emit_off[j+1] <= out_cap, checked on
   the device before any load or store of the frame. */
#ifndef FD_ED25519_EMIT_LAYOUT_H
#define FD_ED25519_EMIT_LAYOUT_H

#include <stdint.h>

#if defined(__HIP__)
#define FD_EMIT_FN static inline __host__ __device__
#else
#define FD_EMIT_FN static inline
#endif

/* Largest message of a signature frame (the engine's largest blob_max) and
   largest payload of a transaction frame (what the u16 holds:
   FD_TXN_AMD_PAYLOAD_MAX).  A larger item has no frame: size 0. */
#define FD_AMD_EMIT_MSG_MAX     (0xFFFFF000u - 96u)
#define FD_AMD_EMIT_PAYLOAD_MAX (65535u)

/* The frame of one item: its size in bytes (the return value) and its
   stride in units of 128 B (*units).  txn == 0: p = the message's bytes.
   txn != 0: p = the payload's bytes, f = the descriptor's footprint. */
FD_EMIT_FN uint32_t
fd_amd_emit_frame( int txn, uint32_t p, uint32_t f, uint32_t * units ) {
  uint32_t sz;
  if( !txn ) sz = p > FD_AMD_EMIT_MSG_MAX ? 0u : 96u + p;
  else       sz = ( p > FD_AMD_EMIT_PAYLOAD_MAX || f > 0xFFF00000u ) ? 0u : ( ( p + 15u ) & ~15u ) + f + 2u;
  *units = (uint32_t)( ( (uint64_t)sz + 127UL ) >> 7 );
  return sz;
}

/* The descriptor bound's arithmetic (fd_txn_amd_desc_bound: the comment there
   derives it), here so that the emit bound is pure host code. */
FD_EMIT_FN uint64_t
fd_amd_desc_bound1( uint64_t payload_sz ) {
  if( payload_sz < 134UL || payload_sz > 65535UL ) return 0UL;
  uint64_t b = 20UL + 10UL*( ( payload_sz - 134UL )/3UL );
  return ( payload_sz <= 1232UL && b > 3570UL ) ? 3570UL : b;
}

#endif /* FD_ED25519_EMIT_LAYOUT_H */

#if defined(FD_ED25519_GATHER_H) && !defined(FD_ED25519_EMIT_KERNELS_H)
#define FD_ED25519_EMIT_KERNELS_H

#define EMIT_G  (4)   /* signature frames in flight per 16-lane group */
#define EMIT_GT (2)   /* transaction frames in flight per 16-lane group (two ranges each) */
#define EMIT_R  (5)   /* batches of 16 aligned words per pass and range: GATHER_R's reason */

/* v with its bytes [k, 16) zeroed; k >= 16 keeps all of it */
FD_DEV uint4
emit_keep_bytes( uint4 v, u32 k ) {
  u32 m[4];
  _Pragma("unroll") for( u32 c=0u; c<4u; c++ ) {
    u32 const kc = k > 4u*c ? min( k - 4u*c, 4u ) : 0u;
    m[c] = kc >= 4u ? 0xFFFFFFFFu : ( ( 1u << ( 8u*kc ) ) - 1u );
  }
  return make_uint4( v.x & m[0], v.y & m[1], v.z & m[2], v.w & m[3] );
}

/* The loads of one pass over a range that starts at s and spans nA aligned
   words: lane j takes words t0 + 16 r + j, r < EMIT_R; word r = EMIT_R is
   the pass's last lane's neighbour and lane 0 alone loads it (k_gather's
   ld_msg). */
FD_DEV void
emit_ld( uint4 (&v)[EMIT_R + 1], u64 s, u32 nA, u32 t0, u32 j, u8 const * idle ) {
  _Pragma("unroll") for( int r=0; r<=EMIT_R; r++ ) {
    u32 const t = t0 + 16u*(u32)r + j;
    v[r] = gather_ld( s, t, t < nA && ( r < EMIT_R || !j ), idle );
  }
}

/* The stores of that pass: output word t, bytes [16 t, 16 t + 16) of the
   range's len bytes and zeros behind them, goes to o[t] for t < nO.  Word tw
   (none: ~0) also takes tv into its 32-bit component tc.  Every lane of the
   wave calls this (the shuffles need them all); nO = 0 stores nothing. */
FD_DEV void
emit_st( uint4 const (&v)[EMIT_R + 1], uint4 * o, u32 sh, u32 len, u32 nO, u32 t0, u32 j, u32 l, u32 tw, u32 tc, u32 tv ) {
  _Pragma("unroll") for( int r=0; r<EMIT_R; r++ ) {
    /* the next aligned word: lane j + 1's of this batch, for lane 15 lane 0's of the next batch */
    uint4 const hi = gather_shfl( j ? v[r] : v[r+1], j == 15u ? l - 15u : l + 1u );
    u32 const t = t0 + 16u*(u32)r + j;
    uint4 w = emit_keep_bytes( gather_shift( v[r], hi, sh ), len > 16u*t ? len - 16u*t : 0u );
    u32 const hit = 0u - (u32)( t == tw );
    w.x |= tv & hit & ( 0u - (u32)( tc == 0u ) );  w.y |= tv & hit & ( 0u - (u32)( tc == 1u ) );
    w.z |= tv & hit & ( 0u - (u32)( tc == 2u ) );  w.w |= tv & hit & ( 0u - (u32)( tc == 3u ) );
    if( t < nO ) o[t] = w;
  }
}

/* Size step, one lane per survivor slot j < n.  cnt = min( *kcnt, n ); for
   j < cnt the item is keep[j], and an item >= n has no frame and is not
   looked up.  Scratch: s_idx[j] the item (~0: none), s_esz[j], s_units[j]
   (0 for j >= cnt), s_bsum[b] the units of block b, *s_cnt = cnt.  Output:
   o_esz[j] for j < cnt. */
template<int TXN> __global__ void __launch_bounds__(64)
k_emit_size( u32 n, u32 const * __restrict__ psz, u64 const * __restrict__ doff, u32 const * __restrict__ keep,
             u64 const * __restrict__ kcnt, u32 * __restrict__ s_idx, u32 * __restrict__ s_esz, u32 * __restrict__ s_units,
             u64 * __restrict__ s_bsum, u64 * __restrict__ s_cnt, u32 * __restrict__ o_esz ) {
  u32 const lane = threadIdx.x, j = blockIdx.x * TXN_PACK_BLOCK + lane;
  u64 const c64 = *kcnt;
  u32 const cnt = c64 < (u64)n ? (u32)c64 : n;
  u32 const i = j < cnt ? keep[j] : 0xFFFFFFFFu;   /* j < cnt <= n: inside keep's n entries */
  bool const live = i < n;
  u32 esz = 0u, units = 0u;
  if( live ) esz = fd_amd_emit_frame( TXN, psz[i], TXN ? (u32)( doff[i + 1u] - doff[i] ) : 0u, &units );
  if( j < n )   { s_idx[j] = esz ? i : 0xFFFFFFFFu; s_esz[j] = esz; s_units[j] = units; }
  if( j < cnt ) o_esz[j] = esz;
  u32 const incl = fd_txn_dev::wave_scan_incl( units, lane );
  if( lane == 63u ) s_bsum[blockIdx.x] = (u64)incl;
  if( !j ) *s_cnt = (u64)cnt;
}

/* Offsets, behind the scan of the block totals (s_bsum[b]: the units before
   block b, *s_total: all of them), lanes j in [0, n]: s_off[j] for j < n and
   o_off[j] for j <= cnt.  Slots at or behind cnt have no units, so theirs is
   the total. */
__global__ void __launch_bounds__(64)
k_emit_off( u32 n, u32 const * __restrict__ s_units, u64 const * __restrict__ s_bsum, u64 const * __restrict__ s_total,
            u64 const * __restrict__ s_cnt, u64 * __restrict__ s_off, u64 * __restrict__ o_off ) {
  u32 const lane = threadIdx.x, j = blockIdx.x * TXN_PACK_BLOCK + lane;
  u32 const u = j < n ? s_units[j] : 0u;
  u32 const incl = fd_txn_dev::wave_scan_incl( u, lane );
  u64 const cnt = *s_cnt;
  u64 const off = ( j < n ? s_bsum[blockIdx.x] + (u64)( incl - u ) : *s_total ) << 7;
  if( j < n ) s_off[j] = off;
  if( (u64)j <= cnt ) o_off[j] = off;
}

/* Store, signature frames: k_gather's shape with the records made from the
   verify planes.  Frame slot jj of group g: item s_idx[jj], at out +
   s_off[jj]; words 0..1 the key (lanes 0..2 load), 2..5 the signature (lanes
   3..7), 6.. the message. */
__global__ void __launch_bounds__(64)
k_emit_sig( u8 const * __restrict__ d_pub, u8 const * __restrict__ d_sig, u32 const * __restrict__ d_moff,
            u8 const * __restrict__ d_blob, u32 const * __restrict__ s_idx, u32 const * __restrict__ s_esz,
            u32 const * __restrict__ s_units, u64 const * __restrict__ s_off, u64 const * __restrict__ s_cnt,
            u8 * __restrict__ out, u64 out_cap ) {
  u32 const l = threadIdx.x, g = l >> 4, j = l & 15u;
  u32 const cnt = (u32)*s_cnt;
  u32 const nblk = (cnt + 4u*EMIT_G - 1u) / (4u*EMIT_G);
  u8 const * const idle = (u8 const *)s_idx;
  for( u32 blk = blockIdx.x; blk < nblk; blk += gridDim.x ) {

  u32 sz[EMIT_G], nA[EMIT_G], nO[EMIT_G];
  u64 pub[EMIT_G], sig[EMIT_G], msg[EMIT_G];
  uint4 * o[EMIT_G];
  bool ok[EMIT_G];
  u32 nOmax = 0u;
  _Pragma("unroll") for( int h=0; h<EMIT_G; h++ ) {
    u32 const jj = blk * (4u*EMIT_G) + 4u*(u32)h + g;
    u32 const js = jj < cnt ? jj : 0u;
    u32 const i = s_idx[js], esz = s_esz[js];
    u64 const off = s_off[js];
    /* the capacity check, before any load or store of the frame */
    ok[h] = jj < cnt && i != 0xFFFFFFFFu && off + ( (u64)s_units[js] << 7 ) <= out_cap;
    u32 const is = ok[h] ? i : 0u;
    sz[h]  = ok[h] ? esz - 96u : 0u;
    pub[h] = (u64)( d_pub + 32UL*is );  sig[h] = (u64)( d_sig + 64UL*is );
    msg[h] = (u64)( d_blob + ( sz[h] ? d_moff[is] : 0u ) );
    o[h]   = (uint4 *)( out + ( ok[h] ? off : 0UL ) );
    nO[h]  = (sz[h] + 15u) >> 4;
    nA[h]  = sz[h] ? (u32)(((u32)msg[h] & 15u) + sz[h] + 15u) >> 4 : 0u;   /* no bytes: no word */
    nOmax  = max( nOmax, nO[h] );
  }

  uint4 hv[EMIT_G], v[EMIT_G][EMIT_R + 1];
  /* pass 0: the keys and signatures beside the first message words */
  _Pragma("unroll") for( int h=0; h<EMIT_G; h++ ) {
    u64 const s  = j < 3u ? pub[h] : sig[h];
    u32 const t  = j < 3u ? j : j - 3u;
    u32 const na = (((u32)s & 15u) + (j < 3u ? 32u : 64u) + 15u) >> 4;
    hv[h] = gather_ld( s, t, ok[h] && j < 8u && t < na, idle );
  }
  _Pragma("unroll") for( int h=0; h<EMIT_G; h++ ) emit_ld( v[h], msg[h], nA[h], 0u, j, idle );
  _Pragma("unroll") for( int h=0; h<EMIT_G; h++ ) {
    uint4 const hi = gather_shfl( hv[h], (l + 1u) & 63u );   /* lanes 2 and 7 take a word they do not use */
    if( ok[h] ) {
      if( j < 2u ) o[h][j] = gather_shift( hv[h], hi, (u32)pub[h] & 15u );
      else if( j >= 3u && j < 7u ) o[h][j - 1u] = gather_shift( hv[h], hi, (u32)sig[h] & 15u );
    }
  }
  _Pragma("unroll") for( int h=0; h<EMIT_G; h++ )
    emit_st( v[h], o[h] + 6, (u32)msg[h] & 15u, sz[h], nO[h], 0u, j, l, 0xFFFFFFFFu, 0u, 0u );
  /* messages past 16 EMIT_R words; wave-uniform trip count (the shuffles need every lane) */
  for( u32 t0 = 16u*EMIT_R; __any( t0 < nOmax ); t0 += 16u*EMIT_R ) {
    _Pragma("unroll") for( int h=0; h<EMIT_G; h++ ) emit_ld( v[h], msg[h], nA[h], t0, j, idle );
    _Pragma("unroll") for( int h=0; h<EMIT_G; h++ )
      emit_st( v[h], o[h] + 6, (u32)msg[h] & 15u, sz[h], nO[h], t0, j, l, 0xFFFFFFFFu, 0u, 0u );
  }

  }
}

/* Store, transaction frames: two ranges per frame, the payload (P bytes to
   word 0) and the descriptor (F bytes to word P16/16, its output F + 2 bytes
   long: the u16 goes into word F >> 4 of it, behind the descriptor's tail). */
__global__ void __launch_bounds__(64)
k_emit_txn( u8 const * __restrict__ d_payload, u32 const * __restrict__ d_toff, u32 const * __restrict__ d_tsz,
            u64 const * __restrict__ d_doff, u8 const * __restrict__ d_desc, u32 const * __restrict__ s_idx,
            u32 const * __restrict__ s_esz, u32 const * __restrict__ s_units, u64 const * __restrict__ s_off,
            u64 const * __restrict__ s_cnt, u8 * __restrict__ out, u64 out_cap ) {
  u32 const l = threadIdx.x, g = l >> 4, j = l & 15u;
  u32 const cnt = (u32)*s_cnt;
  u32 const nblk = (cnt + 4u*EMIT_GT - 1u) / (4u*EMIT_GT);
  u8 const * const idle = (u8 const *)s_idx;
  for( u32 blk = blockIdx.x; blk < nblk; blk += gridDim.x ) {

  u32 P[EMIT_GT], F[EMIT_GT], nAp[EMIT_GT], nOp[EMIT_GT], nAd[EMIT_GT], nOd[EMIT_GT];
  u64 pay[EMIT_GT], dsc[EMIT_GT];
  uint4 * o[EMIT_GT];
  u32 nOpmax = 0u, nOdmax = 0u;
  _Pragma("unroll") for( int h=0; h<EMIT_GT; h++ ) {
    u32 const jj = blk * (4u*EMIT_GT) + 4u*(u32)h + g;
    u32 const js = jj < cnt ? jj : 0u;
    u32 const i = s_idx[js], esz = s_esz[js];
    u64 const off = s_off[js];
    /* the capacity check, before any load or store of the frame */
    bool const ok = jj < cnt && i != 0xFFFFFFFFu && off + ( (u64)s_units[js] << 7 ) <= out_cap;
    u32 const is = ok ? i : 0u;
    P[h] = ok ? d_tsz[is] : 0u;
    u32 const P16 = ( P[h] + 15u ) & ~15u;
    F[h] = ok ? esz - P16 - 2u : 0u;
    pay[h] = (u64)( d_payload + ( P[h] ? d_toff[is] : 0u ) );
    dsc[h] = (u64)( d_desc + ( F[h] ? d_doff[is] : 0UL ) );
    o[h]   = (uint4 *)( out + ( ok ? off : 0UL ) );
    nOp[h] = P16 >> 4;
    nAp[h] = P[h] ? (u32)(((u32)pay[h] & 15u) + P[h] + 15u) >> 4 : 0u;
    nOd[h] = ok ? ( F[h] + 2u + 15u ) >> 4 : 0u;
    nAd[h] = F[h] ? (u32)(((u32)dsc[h] & 15u) + F[h] + 15u) >> 4 : 0u;
    nOpmax = max( nOpmax, nOp[h] );  nOdmax = max( nOdmax, nOd[h] );
  }

  uint4 v[EMIT_GT][EMIT_R + 1], w[EMIT_GT][EMIT_R + 1];
  auto st_pay = [&]( u32 t0 ) {
    _Pragma("unroll") for( int h=0; h<EMIT_GT; h++ )
      emit_st( v[h], o[h], (u32)pay[h] & 15u, P[h], nOp[h], t0, j, l, 0xFFFFFFFFu, 0u, 0u );
  };
  auto st_dsc = [&]( u32 t0 ) {
    _Pragma("unroll") for( int h=0; h<EMIT_GT; h++ )
      emit_st( w[h], o[h] + nOp[h], (u32)dsc[h] & 15u, F[h], nOd[h], t0, j, l,
               nOd[h] ? F[h] >> 4 : 0xFFFFFFFFu, ( F[h] & 15u ) >> 2, P[h] << ( 8u*( F[h] & 2u ) ) );
  };
  /* pass 0: both ranges' first 16 EMIT_R words (any payload up to the MTU; a one-instruction descriptor) */
  _Pragma("unroll") for( int h=0; h<EMIT_GT; h++ ) emit_ld( v[h], pay[h], nAp[h], 0u, j, idle );
  _Pragma("unroll") for( int h=0; h<EMIT_GT; h++ ) emit_ld( w[h], dsc[h], nAd[h], 0u, j, idle );
  st_pay( 0u );
  st_dsc( 0u );
  /* longer ranges; wave-uniform trip counts (the shuffles need every lane) */
  for( u32 t0 = 16u*EMIT_R; __any( t0 < nOpmax ); t0 += 16u*EMIT_R ) {
    _Pragma("unroll") for( int h=0; h<EMIT_GT; h++ ) emit_ld( v[h], pay[h], nAp[h], t0, j, idle );
    st_pay( t0 );
  }
  for( u32 t0 = 16u*EMIT_R; __any( t0 < nOdmax ); t0 += 16u*EMIT_R ) {
    _Pragma("unroll") for( int h=0; h<EMIT_GT; h++ ) emit_ld( w[h], dsc[h], nAd[h], t0, j, idle );
    st_dsc( t0 );
  }

  }
}

fd_amd_emit_layout_t
fd_amd_emit_layout( size_t n ) {
  fd_amd_emit_layout_t L;
  size_t const m = n ? n : 1UL, nblk = ( m + TXN_PACK_BLOCK - 1UL ) / TXN_PACK_BLOCK;
  size_t o = 0;
  L.idx   = o; o = ( o + 4UL*m + 255UL ) & ~(size_t)255UL;
  L.esz   = o; o = ( o + 4UL*m + 255UL ) & ~(size_t)255UL;
  L.units = o; o = ( o + 4UL*m + 255UL ) & ~(size_t)255UL;
  L.off   = o; o = ( o + 8UL*m + 255UL ) & ~(size_t)255UL;
  L.bsum  = o; o = ( o + 8UL*nblk + 255UL ) & ~(size_t)255UL;
  L.word  = o; o += 256UL;   /* the units' total, then cnt */
  L.total = o;
  return L;
}

/* txn == 0: a = d_pub, b = d_sig, c = d_msg_off, psz = d_msg_sz, d = d_blob;
   txn != 0: a = d_payload, c = d_txn_off, psz = d_txn_sz, doff = d_desc_off, d = d_desc */
static int
emit_launch( int txn, u32 n, u8 const * a, u8 const * b, u32 const * c, u32 const * psz, u64 const * doff, u8 const * d,
             u32 const * d_keep, u64 const * d_keep_cnt, u8 * d_out, u64 out_cap, u64 * d_emit_off, u32 * d_emit_sz,
             void * d_scratch, u32 waves, hipStream_t stream ) {
  if( n > FD_AMD_KEEP_MAX ) return -1;
  fd_amd_emit_layout_t L = fd_amd_emit_layout( n );
  u8 * w8 = (u8 *)d_scratch;
  u32 * s_idx = (u32 *)(w8 + L.idx), * s_esz = (u32 *)(w8 + L.esz), * s_units = (u32 *)(w8 + L.units);
  u64 * s_off = (u64 *)(w8 + L.off), * s_bsum = (u64 *)(w8 + L.bsum), * s_total = (u64 *)(w8 + L.word), * s_cnt = s_total + 1;
  u32 const nblk = n ? (n + TXN_PACK_BLOCK - 1u)/TXN_PACK_BLOCK : 1u;
  if( txn ) hipLaunchKernelGGL( k_emit_size<1>, dim3(nblk), dim3(64), 0, stream, n, psz, doff, d_keep, d_keep_cnt, s_idx, s_esz,
                                s_units, s_bsum, s_cnt, d_emit_sz );
  else      hipLaunchKernelGGL( k_emit_size<0>, dim3(nblk), dim3(64), 0, stream, n, psz, doff, d_keep, d_keep_cnt, s_idx, s_esz,
                                s_units, s_bsum, s_cnt, d_emit_sz );
  if( fd_amd_launch_bscan64( nblk, (uint64_t *)s_bsum, (uint64_t *)s_total, stream ) ) return -1;
  hipLaunchKernelGGL( k_emit_off, dim3(n/TXN_PACK_BLOCK + 1u), dim3(64), 0, stream, n, (u32 const *)s_units, (u64 const *)s_bsum,
                      (u64 const *)s_total, (u64 const *)s_cnt, s_off, d_emit_off );
  if( n ) {
    u32 const per = 4u*(u32)( txn ? EMIT_GT : EMIT_G );
    u32 nb = (n + per - 1u)/per;
    if( nb > ( waves ? waves : 65535u ) ) nb = waves ? waves : 65535u;
    if( txn ) hipLaunchKernelGGL( k_emit_txn, dim3(nb), dim3(64), 0, stream, a, c, psz, doff, d, (u32 const *)s_idx,
                                  (u32 const *)s_esz, (u32 const *)s_units, (u64 const *)s_off, (u64 const *)s_cnt, d_out, out_cap );
    else      hipLaunchKernelGGL( k_emit_sig, dim3(nb), dim3(64), 0, stream, a, b, c, d, (u32 const *)s_idx, (u32 const *)s_esz,
                                  (u32 const *)s_units, (u64 const *)s_off, (u64 const *)s_cnt, d_out, out_cap );
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int
fd_amd_launch_emit_sig( uint32_t n, uint8_t const * d_pub, uint8_t const * d_sig, uint32_t const * d_msg_off,
                        uint32_t const * d_msg_sz, uint8_t const * d_blob, uint32_t const * d_keep, uint64_t const * d_keep_cnt,
                        void * d_out, uint64_t out_cap, uint64_t * d_emit_off, uint32_t * d_emit_sz, void * d_scratch,
                        uint32_t waves, hipStream_t stream ) {
  return emit_launch( 0, n, d_pub, d_sig, d_msg_off, d_msg_sz, NULL, d_blob, d_keep, (u64 const *)d_keep_cnt, (u8 *)d_out, out_cap,
                      (u64 *)d_emit_off, d_emit_sz, d_scratch, waves, stream );
}

int
fd_amd_launch_emit_txn( uint32_t txn_cnt, uint8_t const * d_payload, uint32_t const * d_txn_off, uint32_t const * d_txn_sz,
                        uint64_t const * d_desc_off, uint8_t const * d_desc, uint32_t const * d_keep,
                        uint64_t const * d_keep_cnt, void * d_out, uint64_t out_cap, uint64_t * d_emit_off, uint32_t * d_emit_sz,
                        void * d_scratch, uint32_t waves, hipStream_t stream ) {
  return emit_launch( 1, txn_cnt, d_payload, NULL, d_txn_off, d_txn_sz, (u64 const *)d_desc_off, d_desc, d_keep,
                      (u64 const *)d_keep_cnt, (u8 *)d_out, out_cap, (u64 *)d_emit_off, d_emit_sz, d_scratch, waves, stream );
}

#endif /* FD_ED25519_EMIT_KERNELS_H */
