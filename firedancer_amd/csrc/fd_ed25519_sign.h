/* firedancer_amd/csrc/fd_ed25519_sign.h
 *
 * Device functions of the GPU signer (k_sign, fd_ed25519_sign.hip): the
 * prefixed SHA-512, the fixed-base scalar multiplication with its recoding,
 * inversion and encoding, and the scalar multiply-add.  They live in a
 * header so that the probe kernels (tests/hip/fd_probe.hip) can run each of
 * them alone on directed inputs; the signer's kernel and launch code stay in
 * fd_ed25519_sign.hip.
 */
#ifndef FD_ED25519_SIGN_H
#define FD_ED25519_SIGN_H

#include "fd_ed25519_dev.h"

typedef int8_t i8;

namespace {

__device__ static i32 const BASE[32][8][3][10] = FD_AMD_BASE_COMB;

/* SHA-512 over NPRE prefix words (big-endian-loaded u64s, in message byte
   order as little-endian words like k_prep's R||A) followed by M[0..sz) */
template<int NPRE>
__device__ void
sha512_pm( u64 st[8], u64 const pre[NPRE], u8 const * M, u32 sz ) {
  u64 const H0[8] = FD_AMD_SHA512_H0;
  _Pragma("unroll") for( int k=0; k<8; k++ ) st[k] = H0[k];
  u32 nblk = (8u*NPRE + sz + 17u + 127u) / 128u;
  u64 bitlen = (u64)(8u*NPRE + sz) << 3;
  for( u32 blk=0; blk<nblk; blk++ ) {
    u64 w[16];
    _Pragma("unroll") for( int k=0; k<16; k++ ) {
      u32 kk = blk*16u + (u32)k;
      u64 v;
      if( kk < (u32)NPRE ) v = pre[kk < (u32)NPRE ? kk : 0];
      else                 v = msg_word( M, sz, 8u*(kk - (u32)NPRE) );
      v = bswap64( v );
      if( blk == nblk-1u && k == 15 ) v |= bitlen;
      w[k] = v;
    }
    sha512_compress( st, w );
  }
}

/* digest -> 16 little-endian u32 words (the byte string as an integer) */
__device__ __forceinline__ void
digest_words( u32 hd[16], u64 const st[8] ) {
  _Pragma("unroll") for( int a=0; a<8; a++ ) {
    hd[2*a]   = __builtin_bswap32( (u32)(st[a] >> 32) );
    hd[2*a+1] = __builtin_bswap32( (u32)st[a] );
  }
}

/* z^(p-2) by the standard 2^255-21 addition chain (254 squarings) */
__device__ fe
fe_invert( fe const & z ) {
  fe t0 = fe_sq( z );                       /* 2 */
  fe t1 = fe_sq_iter( t0, 2 );              /* 8 */
  t1 = fe_mul( z, t1 );                     /* 9 */
  t0 = fe_mul( t0, t1 );                    /* 11 */
  fe t2 = fe_sq( t0 );                      /* 22 */
  t1 = fe_mul( t1, t2 );                    /* 2^5 - 1 */
  t2 = fe_sq_iter( t1, 5 );  t1 = fe_mul( t2, t1 );     /* 2^10 - 1 */
  t2 = fe_sq_iter( t1, 10 ); t2 = fe_mul( t2, t1 );     /* 2^20 - 1 */
  fe t3 = fe_sq_iter( t2, 20 ); t2 = fe_mul( t3, t2 );  /* 2^40 - 1 */
  t2 = fe_sq_iter( t2, 10 ); t1 = fe_mul( t2, t1 );     /* 2^50 - 1 */
  t2 = fe_sq_iter( t1, 50 ); t2 = fe_mul( t2, t1 );     /* 2^100 - 1 */
  t3 = fe_sq_iter( t2, 100 ); t2 = fe_mul( t3, t2 );    /* 2^200 - 1 */
  t2 = fe_sq_iter( t2, 50 ); t1 = fe_mul( t2, t1 );     /* 2^250 - 1 */
  t1 = fe_sq_iter( t1, 5 );                              /* 2^255 - 2^5 */
  return fe_mul( t1, t0 );                               /* 2^255 - 21 */
}

/* canonical little-endian encoding (limb offsets 0,26,51,...,230) */
__device__ void
fe_tobytes_w( u32 w[8], fe const & f ) {
  i32 h[10];
  fe_reduce( h, f );
  int const off[10] = { 0, 26, 51, 77, 102, 128, 153, 179, 204, 230 };
  _Pragma("unroll") for( int k=0; k<8; k++ ) w[k] = 0u;
  _Pragma("unroll") for( int k=0; k<10; k++ ) {
    u32 v = (u32)h[k];
    int wi = off[k] >> 5, sh = off[k] & 31;
    w[wi] |= v << sh;
    if( sh && wi < 7 ) w[wi+1] |= v >> (32 - sh);
  }
}

struct gp3 { fe X, Y, Z, T; };

/* h += sign*BASE[j][|d|-1] (mixed addition with a Duif-form table entry) */
__device__ __forceinline__ void
madd_base( gp3 & h, int j, int d ) {
  if( !d ) return;
  int a = d < 0 ? -d : d;
  fe ypx, ymx, xy2d;
  _Pragma("unroll") for( int k=0; k<10; k++ ) {
    ypx.v[k] = BASE[j][a-1][0][k]; ymx.v[k] = BASE[j][a-1][1][k]; xy2d.v[k] = BASE[j][a-1][2][k];
  }
  if( d < 0 ) { fe t = ypx; ypx = ymx; ymx = t; xy2d = fe_neg( xy2d ); }
  fe A = fe_mul( fe_add( h.Y, h.X ), ypx );
  fe Bv = fe_mul( fe_sub( h.Y, h.X ), ymx );
  fe C = fe_mul( xy2d, h.T );
  fe D = fe_add( h.Z, h.Z );
  fe X3 = fe_sub( A, Bv ), Y3 = fe_add( A, Bv ), Z3 = fe_add( D, C ), T3 = fe_sub( D, C );
  h.X = fe_mul( X3, T3 ); h.Y = fe_mul( Y3, Z3 ); h.Z = fe_mul( Z3, T3 ); h.T = fe_mul( X3, Y3 );
}

__device__ __forceinline__ void
dbl( gp3 & h ) {
  fe XX = fe_sq( h.X ), YY = fe_sq( h.Y ), B = fe_sqn<2>( h.Z ), A = fe_sq( fe_add( h.X, h.Y ) );
  fe Y3 = fe_add( YY, XX ), Z3 = fe_sub( YY, XX ), X3 = fe_sub( A, Y3 ), T3 = fe_sub( B, Z3 );
  h.X = fe_mul( X3, T3 ); h.Y = fe_mul( Y3, Z3 ); h.Z = fe_mul( Z3, T3 ); h.T = fe_mul( X3, Y3 );
}

/* signed radix-16 digits e[0..63] in [-8,8] of a 256-bit scalar s (8 LE
   words, s < 2^255), packed 4 per word as int8 */
__device__ __forceinline__ void
recode_radix16( u32 dig[16], u32 const s[8] ) {
  int carry = 0;
  _Pragma("unroll") for( int i=0; i<64; i++ ) {
    int e = (int)((s[i >> 3] >> (4 * (i & 7))) & 15u) + carry;
    carry = (e + 8) >> 4;
    e -= carry << 4;
    if( i == 63 ) e += carry << 4;             /* s < 2^255: the top digit absorbs the final carry */
    if( (i & 3) == 0 ) dig[i >> 2] = 0u;
    dig[i >> 2] |= ((u32)(e & 0xff)) << (8 * (i & 3));
  }
}

/* [s]B for a 256-bit scalar s (8 LE words, s < 2^255), encoded */
__device__ void
scalarmult_base_enc( u32 enc[8], u32 const s[8] ) {
  u32 dig[16];
  recode_radix16( dig, s );
  auto D = [&]( int i ) -> int { return (int)(i8)(dig[i >> 2] >> (8 * (i & 3))); };
  gp3 h; h.X = fe_zero(); h.Y = fe_one(); h.Z = fe_one(); h.T = fe_zero();
  for( int i=1; i<64; i+=2 ) madd_base( h, i >> 1, D( i ) );
  dbl( h ); dbl( h ); dbl( h ); dbl( h );
  for( int i=0; i<64; i+=2 ) madd_base( h, i >> 1, D( i ) );
  fe zi = fe_invert( h.Z );
  fe x = fe_mul( h.X, zi ), y = fe_mul( h.Y, zi );
  fe_tobytes_w( enc, y );
  i32 hx[10]; fe_reduce( hx, x );
  enc[7] |= ((u32)hx[0] & 1u) << 31;
}

/* (r + k a) mod L for canonical r, k, a < L (8 LE words each) */
__device__ void
sc_muladd( u32 out[8], u32 const k[8], u32 const a[8], u32 const r[8] ) {
  u32 prod[16];
  _Pragma("unroll") for( int i=0; i<16; i++ ) prod[i] = 0u;
  _Pragma("unroll") for( int i=0; i<8; i++ ) {
    u64 c = 0;
    _Pragma("unroll") for( int j=0; j<8; j++ ) {
      u64 t = (u64)k[i] * a[j] + prod[i+j] + c;
      prod[i+j] = (u32)t; c = t >> 32;
    }
    prod[i+8] = (u32)c;
  }
  u64 c = 0;
  _Pragma("unroll") for( int i=0; i<16; i++ ) {
    u64 t = (u64)prod[i] + (i < 8 ? r[i] : 0u) + c;
    prod[i] = (u32)t; c = t >> 32;
  }
  sc_reduce( out, prod );
}

} /* namespace */

#endif /* FD_ED25519_SIGN_H */
