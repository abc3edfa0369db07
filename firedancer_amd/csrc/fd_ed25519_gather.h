/* firedancer_amd/csrc/fd_ed25519_gather.h -- k_gather: fetch the records of
   a pointer-array chunk from registered host memory into the slot's device
   planes (fd_ed25519_amd_verify_batch_registered); k_gather_txn, below it,
   does the same for the payloads of a transaction chunk
   (fd_ed25519_amd_verify_txns_registered).

   Input: one fd_amd_gather_rec_t per signature, { pub, sig, msg, sz, dst }:
   the device addresses of its 32 public-key, 64 signature and sz message
   bytes and the offset its message gets in the chunk's blob.  Every address
   in a record has one of two sources: the host translated it from the
   registration table (the pointer-array calls), or k_frag_list computed it
   on the device (fd_ed25519_frags.h: inside the one registered data region
   with its whole range, or the slot's own idle block).  Output: d_pub[32 i], d_sig[64 i],
   d_off[i] = dst, d_sz[i] = sz and the message at d_blob + dst -- the planes
   fd_amd_launch_verify reads, as slot_launch_dma fills them.

   Sources have any byte alignment.  A range [s, s + len), len > 0, is read
   as its nA = ((s & 15) + len + 15) >> 4 aligned 16-B words, word t at
   (s & ~15) + 16 t, and output word u (16 B at a 16-aligned destination)
   is bytes [sh, sh + 16), sh = s & 15, of aligned words u | u + 1 -- a
   funnel shift (gather_shift), the ld_words_unaligned idea at 16 B.

   ACCESS INVARIANT.  Every load from caller memory is a naturally aligned
   16-B word that contains at least one byte of the range being copied:
     - word t starts at (s & ~15) + 16 t <= s + 16 t, and it is loaded only
       for t < nA, i.e. 16 t < (s & 15) + len, i.e. its first byte lies
       before s + len; for t = 0 it ends after s, for t > 0 it starts after
       s: so it overlaps [s, s + len);
     - len = 0 loads nothing (nA is forced to 0, whatever s & 15 is);
     - a lane that needs the word after its own (sh != 0) takes it from the
       lane that loaded it (one shuffle), so no word is loaded twice and no
       lane loads a word "just in case";
     - a lane with no such word to fetch in some load instruction (t >= nA)
       loads the first 16 B of d_blob instead -- the slot's own device
       memory, the value never used for a byte that counts (gather_ld).  That keeps the kernel free
       of branches: around a predicated load the compiler branches, and
       after such a branch it waits with vmcnt(0) for loads still on their
       way, which put the keys' round trip in front of the messages'.
   An aligned 16-B word never straddles a page, so no access leaves a page
   the range touches: a record flush against the first or last byte of a
   registration is read without touching the neighbouring pages.  Bytes of
   such a word outside the range (at most 15 before and 15 after) are read
   and, behind a message's last byte, land in that message's own padding in
   d_blob; nothing interprets them.

   Destinations: dst is a multiple of 16 and a message owns
   [dst, dst + round_up( sz, 16 )) of d_blob (fd_ed25519_amd_gather_layout),
   so whole 16-B stores never touch a neighbour; d_blob keeps its 64-B tail
   slack.  The records themselves are 32 B, 32-aligned.

   Shape (after tile_gather): 16 lanes per record; lane j takes aligned
   words j, j + 16, ... of the message, and of the fixed-size ranges lanes
   0..2 the public key's (<= 3) words and lanes 3..7 the signature's (<= 5).
   Each 16-lane group has GATHER_G records in flight and every load of a
   pass -- the key, the signature and the first 16 GATHER_R aligned words
   (1280 B: any message up to the 1232-B MTU, which spans at most 78) of
   all of them -- is issued
   before the first store: the sources are host memory over PCIe, and a
   wave then waits one round trip per pass, not one per record.  Longer
   messages take further passes of the same loop, bounded by
   sz <= blob_max.  A wave takes blocks of 4 GATHER_G records gridDim.x
   apart, so the launch's grid, not n, bounds the host-memory reads in
   flight (the engine caps it where other kernels run beside this one:
   slot_launch_gather).  No atomics, no spinning, vector stores only. */
#ifndef FD_ED25519_GATHER_H
#define FD_ED25519_GATHER_H

#define GATHER_G (4)   /* records in flight per 16-lane group: 16 per wave */
#define GATHER_R (5)   /* batches of 16 aligned message words per pass */

typedef u32 gather_w4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) gather_w4 const * gather_src_t;   /* global, not flat, loads */

/* bytes [sh, sh + 16) of the 32 bytes lo | hi, sh < 16 */
FD_DEV uint4
gather_shift( uint4 lo, uint4 hi, u32 sh ) {
  u32 const d[8] = { lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w };
  /* bit selects (v_bfi_b32), not ?: -- the compiler turns a chain of those
     into a dynamically indexed array in scratch */
  u32 const m1 = 0u - ((sh >> 2) & 1u), m2 = 0u - ((sh >> 3) & 1u);
  u32 f[7], e[5];
  _Pragma("unroll") for( int m=0; m<7; m++ ) f[m] = (d[m+1] & m1) | (d[m] & ~m1);
  _Pragma("unroll") for( int m=0; m<5; m++ ) e[m] = (f[m+2] & m2) | (f[m] & ~m2);   /* e[m] = d[m + (sh >> 2)] */
  u32 const r = sh & 3u;
  return make_uint4( __builtin_amdgcn_alignbyte( e[1], e[0], r ), __builtin_amdgcn_alignbyte( e[2], e[1], r ),
                     __builtin_amdgcn_alignbyte( e[3], e[2], r ), __builtin_amdgcn_alignbyte( e[4], e[3], r ) );
}

FD_DEV uint4
gather_shfl( uint4 v, u32 lane ) {
  return make_uint4( (u32)__shfl( (int)v.x, (int)lane ), (u32)__shfl( (int)v.y, (int)lane ),
                     (u32)__shfl( (int)v.z, (int)lane ), (u32)__shfl( (int)v.w, (int)lane ) );
}

/* take (the caller's t < nA: the access invariant): aligned word t of the
   range that starts at s; else the load goes to `idle`, 16 B of device
   memory, and the lane gets whatever is there.  Not zeros on purpose: a
   select on the result lets the compiler see that the load is needed under
   `take` alone, and it branches around it again.  No byte of an idle lane's
   word reaches a key, a signature or message bytes [0, sz): it is the
   neighbour word only of a lane whose own word already ends the range. */
FD_DEV uint4
gather_ld( u64 s, u32 t, bool take, u8 const * idle ) {
  u64 const a = take ? (s & ~(u64)15) + 16UL*t : (u64)idle;
  gather_w4 const w = *(gather_src_t)a;
  return make_uint4( w.x, w.y, w.z, w.w );
}

__global__ void __launch_bounds__(64)
k_gather( u32 n, fd_amd_gather_rec_t const * __restrict__ rec, u8 * __restrict__ d_pub, u8 * __restrict__ d_sig,
          u32 * __restrict__ d_off, u32 * __restrict__ d_sz, u8 * __restrict__ d_blob ) {
  u32 const l = threadIdx.x, g = l >> 4, j = l & 15u;
  u32 const nblk = (n + 4u*GATHER_G - 1u) / (4u*GATHER_G);
  /* a wave takes blocks of 4 GATHER_G records, gridDim.x apart: the grid, not n, bounds the reads in flight */
  for( u32 blk = blockIdx.x; blk < nblk; blk += gridDim.x ) {

  /* the group's records: record h of group g is signature 4 GATHER_G block + 4 h + g */
  u32 idx[GATHER_G], sz[GATHER_G], dst[GATHER_G], nA[GATHER_G], nO[GATHER_G];
  u64 pub[GATHER_G], sig[GATHER_G], msg[GATHER_G];
  u32 nOmax = 0u;
  _Pragma("unroll") for( int h=0; h<GATHER_G; h++ ) {
    idx[h] = blk * (4u*GATHER_G) + 4u*(u32)h + g;
    bool const live = idx[h] < n;
    uint4 const * rp = (uint4 const *)(rec + (live ? idx[h] : 0u));
    uint4 const r0 = rp[0], r1 = rp[1];
    pub[h] = ((u64)r0.y << 32) | r0.x;  sig[h] = ((u64)r0.w << 32) | r0.z;  msg[h] = ((u64)r1.y << 32) | r1.x;
    sz[h] = live ? r1.z : 0u;  dst[h] = r1.w;
    if( !live ) idx[h] = 0xFFFFFFFFu;
    nO[h] = (sz[h] + 15u) >> 4;                                         /* sz <= blob_max < 2^32 - 4096 */
    nA[h] = sz[h] ? (u32)(((u32)msg[h] & 15u) + sz[h] + 15u) >> 4 : 0u;  /* no bytes: no word */
    nOmax = max( nOmax, nO[h] );
  }

  uint4 hv[GATHER_G], v[GATHER_G][GATHER_R + 1];
  /* one pass over aligned message words [t0, t0 + 16 GATHER_R] of every record: its loads, then its stores */
  auto ld_msg = [&]( u32 t0 ) {
    _Pragma("unroll") for( int h=0; h<GATHER_G; h++ ) {
      _Pragma("unroll") for( int r=0; r<=GATHER_R; r++ ) {
        u32 const t = t0 + 16u*(u32)r + j;
        /* word r = GATHER_R is the pass's last lane's neighbour: lane 0 alone loads it */
        v[h][r] = gather_ld( msg[h], t, t < nA[h] && ( r < GATHER_R || !j ), d_blob );
      }
    }
  };
  auto st_msg = [&]( u32 t0 ) {
    _Pragma("unroll") for( int h=0; h<GATHER_G; h++ ) {
      uint4 * const o = (uint4 *)(d_blob + dst[h]);
      u32 const sh = (u32)msg[h] & 15u;
      _Pragma("unroll") for( int r=0; r<GATHER_R; r++ ) {
        /* the next aligned word: lane j + 1's of this batch, for lane 15 lane 0's of the next batch */
        uint4 const hi = gather_shfl( j ? v[h][r] : v[h][r+1], j == 15u ? l - 15u : l + 1u );
        u32 const t = t0 + 16u*(u32)r + j;
        if( t < nO[h] ) o[t] = gather_shift( v[h][r], hi, sh );
      }
    }
  };

  /* pass 0, outside the loop (a loop head would wait for the keys and
     signatures before it issues the message loads): the keys and signatures
     beside the first message words */
  _Pragma("unroll") for( int h=0; h<GATHER_G; h++ ) {
    /* lanes 0..2: the key's aligned words (2, or 3 when it is not 16-aligned); lanes 3..7: the signature's (4 or 5) */
    bool const live = idx[h] != 0xFFFFFFFFu;
    u64 const s  = j < 3u ? pub[h] : sig[h];
    u32 const t  = j < 3u ? j : j - 3u;
    u32 const na = (((u32)s & 15u) + (j < 3u ? 32u : 64u) + 15u) >> 4;
    hv[h] = gather_ld( s, t, live && j < 8u && t < na, d_blob );
  }
  ld_msg( 0u );
  _Pragma("unroll") for( int h=0; h<GATHER_G; h++ ) {
    uint4 const hi = gather_shfl( hv[h], (l + 1u) & 63u );   /* lanes 2 and 7 take a word they do not use */
    if( idx[h] != 0xFFFFFFFFu ) {
      if( j < 2u ) ((uint4 *)(d_pub + 32UL*idx[h]))[j] = gather_shift( hv[h], hi, (u32)pub[h] & 15u );
      else if( j >= 3u && j < 7u ) ((uint4 *)(d_sig + 64UL*idx[h]))[j - 3u] = gather_shift( hv[h], hi, (u32)sig[h] & 15u );
      else if( j == 8u ) { d_off[idx[h]] = dst[h]; d_sz[idx[h]] = sz[h]; }
    }
  }
  st_msg( 0u );
  /* messages past 16 GATHER_R words; wave-uniform trip count (the shuffles need every lane), bounded by sz <= blob_max */
  for( u32 t0 = 16u*GATHER_R; __any( t0 < nOmax ); t0 += 16u*GATHER_R ) { ld_msg( t0 ); st_msg( t0 ); }

  }
}

/* k_gather_txn: fetch the payloads of a pointer-array transaction chunk from
   registered host memory into the slot's device blob and write the chunk's
   transaction planes (fd_ed25519_amd_verify_txns_registered).

   Input: one fd_amd_gather_txn_rec_t per transaction, { src, sz, dst, tbase }:
   the device address of its sz payload bytes (translated on the host from
   the registration table, the only source of addresses this kernel is ever
   given), the offset the payload gets in d_blob and its first signature
   slot.  Output: the payload at d_blob + dst, d_toff[t] = dst, d_tsz[t] = sz,
   d_tbase[t] = tbase and d_tbase[n] = slot_cnt (a kernel argument) -- what
   k_txn_parse, k_txn_reduce and k_tag_gather read, so the chunk needs no
   host-to-device copy.

   ACCESS INVARIANT.  Every load from caller memory is a naturally aligned
   16-B word that contains at least one byte of the range being copied:
     - word t starts at (s & ~15) + 16 t <= s + 16 t, and it is loaded only
       for t < nA, i.e. 16 t < (s & 15) + len, i.e. its first byte lies
       before s + len; for t = 0 it ends after s, for t > 0 it starts after
       s: so it overlaps [s, s + len);
     - len = 0 loads nothing (nA is forced to 0, whatever s & 15 is);
     - a lane that needs the word after its own (sh != 0) takes it from the
       lane that loaded it (one shuffle), so no word is loaded twice and no
       lane loads a word "just in case";
     - a lane with no such word to fetch in some load instruction (t >= nA)
       loads the first 16 B of d_blob instead -- the slot's own device
       memory, the value never used for a byte that counts (gather_ld).  That keeps the kernel free
       of branches: around a predicated load the compiler branches, and
       after such a branch it waits with vmcnt(0) for loads still on their
       way.
   An aligned 16-B word never straddles a page, so a payload flush against
   the first or last byte of a registration is read without touching the
   neighbouring pages.  Bytes of such a word outside the range (at most 15
   before and 15 after) are read and, behind a payload's last byte, land in
   that payload's own padding in d_blob; the parser reads [dst, dst + sz)
   alone.

   Destinations: dst is a multiple of 16 and a payload owns
   [dst, dst + round_up( sz, 16 )) of d_blob
   (fd_ed25519_amd_txn_gather_layout), so whole 16-B stores never touch a
   neighbour; d_blob keeps its 64-B tail slack.

   Shape: k_gather's.  16 lanes per record, lane j takes aligned words j,
   j + 16, ...; each 16-lane group has GATHER_G records in flight and every
   load of them is issued before the first store; a wave takes blocks of
   4 GATHER_G records gridDim.x apart, so the grid bounds the host-memory
   reads in flight.  ONE pass: a payload is at most FD_TXN_AMD_MTU bytes,
   which span at most 78 aligned words, and the pass loads 16 GATHER_R = 80.
   The entry point is the only producer of records and has refused larger
   sizes, so there is no further-pass loop (a larger sz would be copied
   short, never out of bounds: stores stay below word 16 GATHER_R of the
   payload's own, then larger, range).  Output word u < nO takes aligned
   words u and u + 1; u + 1 is a word of the range only when u + 1 < nA <=
   16 GATHER_R, so no lane needs a word past the pass (k_gather's extra word
   GATHER_R is not loaded).  No atomics, no spinning, vector stores only. */
static_assert( ((15UL + FD_TXN_AMD_MTU + 15UL) >> 4) <= 16UL*GATHER_R,
               "k_gather_txn copies a payload in one pass of 16 GATHER_R aligned words" );

__global__ void __launch_bounds__(64)
k_gather_txn( u32 n, fd_amd_gather_txn_rec_t const * __restrict__ rec, u8 * __restrict__ d_blob, u32 * __restrict__ d_toff,
              u32 * __restrict__ d_tsz, u32 * __restrict__ d_tbase, u32 slot_cnt ) {
  u32 const l = threadIdx.x, g = l >> 4, j = l & 15u;
  u32 const nblk = (n + 4u*GATHER_G - 1u) / (4u*GATHER_G);
  if( !blockIdx.x && !l ) d_tbase[n] = slot_cnt;
  /* a wave takes blocks of 4 GATHER_G records, gridDim.x apart: the grid, not n, bounds the reads in flight */
  for( u32 blk = blockIdx.x; blk < nblk; blk += gridDim.x ) {

  /* the group's records: record h of group g is transaction 4 GATHER_G block + 4 h + g */
  u32 idx[GATHER_G], sz[GATHER_G], dst[GATHER_G], tb[GATHER_G], nA[GATHER_G], nO[GATHER_G];
  u64 src[GATHER_G];
  _Pragma("unroll") for( int h=0; h<GATHER_G; h++ ) {
    idx[h] = blk * (4u*GATHER_G) + 4u*(u32)h + g;
    bool const live = idx[h] < n;
    uint4 const * rp = (uint4 const *)(rec + (live ? idx[h] : 0u));
    uint4 const r0 = rp[0], r1 = rp[1];
    src[h] = ((u64)r0.y << 32) | r0.x;
    sz[h] = live ? r0.z : 0u;  dst[h] = r0.w;  tb[h] = r1.x;
    if( !live ) idx[h] = 0xFFFFFFFFu;
    nO[h] = (sz[h] + 15u) >> 4;                                         /* sz <= FD_TXN_AMD_MTU */
    nA[h] = sz[h] ? (u32)(((u32)src[h] & 15u) + sz[h] + 15u) >> 4 : 0u;  /* no bytes: no word */
  }

  /* aligned words [0, 16 GATHER_R) of every record: the loads, then the stores */
  uint4 v[GATHER_G][GATHER_R];
  _Pragma("unroll") for( int h=0; h<GATHER_G; h++ ) {
    _Pragma("unroll") for( int r=0; r<GATHER_R; r++ ) {
      u32 const t = 16u*(u32)r + j;
      v[h][r] = gather_ld( src[h], t, t < nA[h], d_blob );
    }
  }
  _Pragma("unroll") for( int h=0; h<GATHER_G; h++ ) {
    uint4 * const o = (uint4 *)(d_blob + dst[h]);
    u32 const sh = (u32)src[h] & 15u;
    _Pragma("unroll") for( int r=0; r<GATHER_R; r++ ) {
      /* the next aligned word: lane j + 1's of this batch, for lane 15 lane 0's of the next batch
         (the last batch has none: its lane 15 is word 16 GATHER_R - 1 >= nO, never stored) */
      uint4 give = v[h][r];
      if( r + 1 < GATHER_R ) {   /* compile time; bit selects, not ?: (gather_shift) */
        uint4 const nx = v[h][r + 1 < GATHER_R ? r + 1 : r];
        u32 const m = 0u - (u32)!j;
        give = make_uint4( (nx.x & m) | (give.x & ~m), (nx.y & m) | (give.y & ~m), (nx.z & m) | (give.z & ~m), (nx.w & m) | (give.w & ~m) );
      }
      uint4 const hi = gather_shfl( give, j == 15u ? l - 15u : l + 1u );
      u32 const t = 16u*(u32)r + j;
      if( t < nO[h] ) o[t] = gather_shift( v[h][r], hi, sh );
    }
    if( !j && idx[h] != 0xFFFFFFFFu ) { d_toff[idx[h]] = dst[h]; d_tsz[idx[h]] = sz[h]; d_tbase[idx[h]] = tb[h]; }
  }

  }
}

#endif
