/* firedancer_amd/csrc/fd_ed25519_front.h
 *
 * The front of the pipeline: slide recoding, SHA-512 and k_prep; k_decomp;
 * k_front (both in one launch).  fd_ed25519_tile.h includes it for the two
 * bodies (prep_body, decomp_body).
 */

#ifndef FD_ED25519_FRONT_H
#define FD_ED25519_FRONT_H

#include "fd_ed25519_ws.h"

/* ------------------------------------------------------------------ */
/* k_prep                                                               */

/* fd_ed25519_ge_slide (avx/fd_ed25519_ge.c:378-400) on a 256-bit register
   shift window: bit 0 of w0 is always position `pos`, so every look-ahead
   index is static.  The reference's carry loop "for k>=i+b: if !r[k] set,
   break; else clear" is the big-integer increment B += 2^(i+b).  Scalars
   are < 2^253 so no carry leaves position 255.  emit(pos, digit). */
template<typename EMIT>
__device__ __forceinline__ void
slide_reg( u32 const a[8], EMIT emit ) {
  u64 w0 = ((u64)a[1] << 32) | a[0], w1 = ((u64)a[3] << 32) | a[2];
  u64 w2 = ((u64)a[5] << 32) | a[4], w3 = ((u64)a[7] << 32) | a[6];
  int pos = 0;
  while( (w0 | w1 | w2 | w3) != 0UL ) {
    /* skip to the next set bit */
    while( w0 == 0UL ) { w0 = w1; w1 = w2; w2 = w3; w3 = 0UL; pos += 64; }
    int tz = __builtin_ctzll( w0 );
    if( tz ) {
      w0 = (w0 >> tz) | (w1 << (64 - tz));
      w1 = (w1 >> tz) | (w2 << (64 - tz));
      w2 = (w2 >> tz) | (w3 << (64 - tz));
      w3 = (w3 >> tz);
      pos += tz;
    }
    int r = 1; w0 &= ~1UL;
    bool stop = false;
    _Pragma("unroll")
    for( int b=1; b<=6; b++ ) {
      bool bit = !stop && ((w0 >> b) & 1UL);
      if( bit ) {
        if( r + (1 << b) <= 15 ) { r += 1 << b; w0 &= ~(1UL << b); }
        else if( r - (1 << b) >= -15 ) {
          r -= 1 << b;
          u64 n0 = w0 + (1UL << b);                 /* B += 2^b (carry chain) */
          u64 c  = n0 < w0;
          w0 = n0; w1 += c; c = c && w1 == 0UL; w2 += c; c = c && w2 == 0UL; w3 += c;
        } else stop = true;
      }
    }
    emit( pos, r );
    /* step past pos */
    w0 = (w0 >> 1) | (w1 << 63); w1 = (w1 >> 1) | (w2 << 63); w2 = (w2 >> 1) | (w3 << 63); w3 >>= 1;
    pos += 1;
  }
}

__device__ __forceinline__ void
prep_body( u32 i, u32 n, u8 const * __restrict__ pub, u8 const * __restrict__ sig,
           u32 const * __restrict__ msg_off, u32 const * __restrict__ msg_sz,
           u8 const * __restrict__ blob, i8 * __restrict__ err, u8 * __restrict__ ws, ws_layout_t L,
           i8 const * __restrict__ skip ) {
  if( i >= n ) return;
  if( skip && skip[i] ) {   /* slot of a transaction that failed to parse (fd_txn_kernels.hip) */
    ((int *)(ws + L.top))[i] = -1;
    ((u32 *)(ws + L.evn))[i] = 0u;
    ((u64 *)(ws + L.tag))[i] = 0UL;
    err[i] = (i8)skip[i];
    return;
  }

  /* R || A as 16 LE dwords (sig / pub records are 64- / 32-byte aligned) */
  uint4 const * S4 = (uint4 const *)(sig + 64UL*i);
  uint4 const * P4 = (uint4 const *)(pub + 32UL*i);
  uint4 r0 = S4[0], r1 = S4[1], s0 = S4[2], s1 = S4[3], a0 = P4[0], a1 = P4[1];
  u32 sw[8] = { s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w };

  /* s-range check with the reference's early "return 0" window (user.c:373-379) */
  int code = 1;   /* pending */
  {
    u32 s31 = sw[7] >> 24;
    if( s31 > 0x10u ) code = -1;
    else if( s31 == 0x10u ) {
      if( (sw[4] | sw[5] | sw[6] | (sw[7] & 0x00ffffffu)) != 0u ) code = 0;   /* s[16..30] != 0 */
      else {
        /* s[0..15] vs l_low, compared from the top byte: s < l_low passes */
        u32 const ll[4] = { 0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu };
        bool less = false, decided = false;
        _Pragma("unroll") for( int k=3; k>=0; k-- ) {
          if( !decided && sw[k] != ll[k] ) { less = sw[k] < ll[k]; decided = true; }
        }
        if( !less ) code = -1;
      }
    }
  }

  u64 * evw = (u64 *)(ws + L.dig) + (size_t)i*32u;   /* this signature's event row: 16 words h, 16 words s */
  u32 nh = 0u, ns = 0u;
  int top = -1;
  u64 tag = 0UL;
  u64 st[8] = FD_AMD_SHA512_H0;
  if( code >= 0 ) {   /* pending, or accepted by the s window (the tag is still the hash) */
    u32 sz = msg_sz[i];
    u8 const * M = blob + msg_off[i];
    u32 nblk = (64u + sz + 17u + 127u) / 128u;
    u64 const ra[8] = { ((u64)r0.y << 32) | r0.x, ((u64)r0.w << 32) | r0.z, ((u64)r1.y << 32) | r1.x, ((u64)r1.w << 32) | r1.z,
                        ((u64)a0.y << 32) | a0.x, ((u64)a0.w << 32) | a0.z, ((u64)a1.y << 32) | a1.x, ((u64)a1.w << 32) | a1.z };
    u64 bitlen = (u64)(64u + sz) << 3;
    for( u32 blk=0; blk<nblk; blk++ ) {
      u64 w[16];
      _Pragma("unroll") for( int k=0; k<16; k++ ) {
        u32 kk = blk*16u + (u32)k;                 /* stream word index */
        u64 v;
        if( kk < 8u ) v = ra[k & 7];               /* only block 0 */
        else          v = msg_word( M, sz, 8u*(kk - 8u) );
        v = bswap64( v );
        if( blk == nblk-1u && k == 15 ) v |= bitlen;
        w[k] = v;
      }
      sha512_compress( st, w );
    }
    tag = bswap64( st[0] );
  }
  if( code == 1 ) {
    u32 hd[16];
    _Pragma("unroll") for( int a=0; a<8; a++ ) {
      hd[2*a]   = __builtin_bswap32( (u32)(st[a] >> 32) );
      hd[2*a+1] = __builtin_bswap32( (u32)st[a] );
    }
    u32 h[8];
    sc_reduce( h, hd );

    /* digits as sparse EVENTS, u16 = position | digit << 8, ascending, four
       per 64-bit word (the consumer walks them from the top).  Consecutive
       nonzero digits of the slide are >= 5 positions apart (bits i+1..i+4
       are always absorbed), so a 253-bit scalar has at most 52 events: the
       16-word halves never overflow.  Only the words holding events are
       written -- no dense 256-entry row, no zero fill. */
    u64 buf = 0UL;
    slide_reg( h, [&]( int pos, int r ) {
      buf |= (u64)((u32)pos | ((u32)(u8)(i8)r << 8)) << (16u*(nh & 3u));
      if( !(++nh & 3u) ) { evw[(nh >> 2) - 1u] = buf; buf = 0UL; }
      top = max( top, pos );
    } );
    if( nh & 3u ) evw[nh >> 2] = buf;
    buf = 0UL;
    slide_reg( sw, [&]( int pos, int r ) {
      buf |= (u64)((u32)pos | ((u32)(u8)(i8)r << 8)) << (16u*(ns & 3u));
      if( !(++ns & 3u) ) { evw[16u + (ns >> 2) - 1u] = buf; buf = 0UL; }
      top = max( top, pos );
    } );
    if( ns & 3u ) evw[16u + (ns >> 2)] = buf;
  }
  ((u32 *)(ws + L.evn))[i] = nh | (ns << 8);
  ((int *)(ws + L.top))[i] = top;
  ((u64 *)(ws + L.tag))[i] = tag;
  err[i] = (i8)code;
}

__global__ void __launch_bounds__(64)
k_prep( u32 n, u8 const * __restrict__ pub, u8 const * __restrict__ sig,
        u32 const * __restrict__ msg_off, u32 const * __restrict__ msg_sz,
        u8 const * __restrict__ blob, i8 * __restrict__ err, u8 * __restrict__ ws, ws_layout_t L,
        i8 const * __restrict__ skip ) {
  prep_body( blockIdx.x * 64u + threadIdx.x, n, pub, sig, msg_off, msg_sz, blob, err, ws, L, skip );
}

/* ------------------------------------------------------------------ */
/* k_decomp: lane 2i -> A = pub[i], lane 2i+1 -> R = sig[i][0:32]       */

#define FD_DECOMP_WAVES 2   /* k_decomp / k_front occupancy target (222 VGPRs) */
/* one point per lane: t = 2i (A = pub[i]) or 2i+1 (R = sig[i][0:32]).
   Independent of k_prep (reads no verdict) when `gate` is 0, so the two
   can run concurrently (k_front); with gate, signatures k_prep already
   decided are skipped. */
__device__ __forceinline__ void
decomp_body( u32 t, u32 n, u8 const * __restrict__ pub, u8 const * __restrict__ sig,
             i8 const * __restrict__ err, u8 * __restrict__ ws, ws_layout_t L, bool gate ) {
  u32 i = t >> 1; u32 which = t & 1u;
  if( i >= n ) return;
  if( gate && err[i] != 1 ) return;
  u8 * ds = ws + L.ds;
  /* the point as 8 LE dwords in two 16-B loads (sig / pub records are 64- /
     32-byte aligned, as k_prep reads them; on the latency path these are
     reads over PCIe from host memory, so fewer, wider loads) */
  uint4 const * src = (uint4 const *)(which ? (sig + 64UL*i) : (pub + 32UL*i));
  uint4 const s0 = src[0], s1 = src[1];
  u32 const w[8] = { s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w };

  fe const D = {FD_AMD_FE_D};
  fe const SQRTM1 = {FD_AMD_FE_SQRTM1};

  fe Y = fe_frombytes( w );
  fe u = fe_sq( Y );
  fe v = fe_mul( u, D );
  u.v[0] -= 1;                      /* u = y^2-1 */
  v.v[0] += 1;                      /* v = dy^2+1 */
  fe v3 = fe_sq( v ); v3 = fe_mul( v3, v );          /* v^3 */
  fe x = fe_sq( v3 ); x = fe_mul( x, v ); x = fe_mul( x, u );   /* uv^7 */
  x = fe_pow22523( x );
  x = fe_mul( x, v3 ); x = fe_mul( x, u );          /* uv^3 (uv^7)^((p-5)/8) */
  fe vxx = fe_sq( x ); vxx = fe_mul( vxx, v );
  fe chk = fe_sub( vxx, u );
  if( fe_isnonzero( chk ) ) {
    chk = fe_add( vxx, u );
    if( fe_isnonzero( chk ) ) { ds[2u*i + which] = 1u; return; }
    x = fe_mul( x, SQRTM1 );
  }
  if( fe_isnegative( x ) != (int)(w[7] >> 31) ) x = fe_neg( x );
  fe T = fe_mul( x, Y );

  size_t N = L.N;
  if( !which ) {
    i32 * A = (i32 *)(ws + L.A);
    fe nx = fe_neg( x ), nt = fe_neg( T );     /* A := -A (user.c:406-407) */
    _Pragma("unroll") for( int k=0; k<10; k++ ) {
      A[(size_t)(k   )*N + i] = nx.v[k];
      A[(size_t)(10+k)*N + i] = Y.v[k];
      A[(size_t)(20+k)*N + i] = nt.v[k];
    }
  } else {
    i32 * R = (i32 *)(ws + L.R);
    _Pragma("unroll") for( int k=0; k<10; k++ ) {
      R[(size_t)(k   )*N + i] = x.v[k];
      R[(size_t)(10+k)*N + i] = Y.v[k];
    }
  }
  ds[2u*i + which] = 0u;
}

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(FD_DECOMP_WAVES)))
k_decomp( u32 n, u8 const * __restrict__ pub, u8 const * __restrict__ sig,
          i8 * __restrict__ err, u8 * __restrict__ ws, ws_layout_t L ) {
  decomp_body( blockIdx.x * 64u + threadIdx.x, n, pub, sig, err, ws, L, true );
}

/* k_front: k_prep and k_decomp as ONE launch, blocks [0, nbp) hashing and
   blocks [nbp, 3 nbp) decompressing, concurrently (latency path: a small
   batch does not fill the GPU, so the two stages overlap instead of
   queueing). */
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(FD_DECOMP_WAVES)))
k_front( u32 n, u32 nbp, u8 const * __restrict__ pub, u8 const * __restrict__ sig,
         u32 const * __restrict__ msg_off, u32 const * __restrict__ msg_sz,
         u8 const * __restrict__ blob, i8 * __restrict__ err, u8 * __restrict__ ws, ws_layout_t L,
         i8 const * __restrict__ skip ) {
  if( blockIdx.x < nbp ) prep_body( blockIdx.x * 64u + threadIdx.x, n, pub, sig, msg_off, msg_sz, blob, err, ws, L, skip );
  else                   decomp_body( (blockIdx.x - nbp) * 64u + threadIdx.x, n, pub, sig, err, ws, L, false );
}

#endif /* FD_ED25519_FRONT_H */
