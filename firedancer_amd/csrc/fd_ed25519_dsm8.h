/* firedancer_amd/csrc/fd_ed25519_dsm8.h
 *
 * The half-multiply (half_ctx, fe5, fe_mul_half5) and k_dsm8, eight lanes
 * per signature.  Included by fd_ed25519_tile.h.
 */

#ifndef FD_ED25519_DSM8_H
#define FD_ED25519_DSM8_H

#include "fd_ed25519_dsm4.h"

/* ------------------------------------------------------------------ */
/* k_dsm8: k_dsm4's op stream on EIGHT lanes per signature (8 signatures per
 * wave): two lane quads hold the same state, and every field mul of the
 * step is split between lane l (h = 0, even columns) and lane l ^ 4 (h = 1,
 * odd columns), 50 products each, so one step issues half the
 * multiply-accumulates per lane.  The instruction stream stays uniform:
 * lane h = 1 sees G shifted down one limb (G[j] = g_{j+1}, its wrap entry
 * G19[9] = g_0) and F undoubled, so slot (c, i) of both halves is
 * f_i * g_{2c+h-i} with that column's reference factors (x2 when i and j are
 * odd, x19 when i + j >= 10, on the wrapped int32 pre-multiples).  The five
 * 64-bit column sums are swapped between the two lanes with DPP
 * row_shl/row_shr 4 under bank masks, and the pair finishes the reference
 * carry chain on pre-biased sums, each lane running one of its two
 * interleaved runs (fe_mul_half5): the same limbs as fe_mul. */
struct half_t { u64 mH; i32 shF; i64 bias; i64 m4, k5; u32 shz, mo0; i32 bo0; };
__device__ __forceinline__ half_t half_ctx( int hh ) {
  half_t H;
  H.mH = __builtin_amdgcn_ballot_w64( hh != 0 );
  H.shF = hh ? 0 : 1;
  H.bias = hh ? (1L<<24) : (1L<<25);
  H.m4  = hh ? -1L : (1L<<26) - 1;           /* split carry (fe_mul_half5): see there */
  H.k5  = hh ? -1L : 0L;
  H.shz = hh ? 25u : 0u;
  H.mo0 = hh ? (1u<<25) - 1u : (1u<<26) - 1u;
  H.bo0 = hh ? (1<<24) : (1<<25);
  asm( "" : "+v"(H.shF), "+v"(H.m4), "+v"(H.k5), "+v"(H.shz), "+v"(H.mo0), "+v"(H.bo0) );
  return H;
}

/* the partner lane's value (lane l ^ 4 of the 8-lane group) where `mine`
   is the h = 0 / h = 1 slot: E keeps h = 0's own value and takes the partner's
   on h = 1 lanes, O the other way round */
__device__ __forceinline__ u32 half_from_lo( u32 v ) {   /* h = 1 lanes read lane - 4 (banks 1, 3) */
  return (u32)__builtin_amdgcn_update_dpp( (int)v, (int)v, 0x114, 0xf, 0xa, false );
}
__device__ __forceinline__ u32 half_from_hi( u32 v ) {   /* h = 0 lanes read lane + 4 (banks 0, 2) */
  return (u32)__builtin_amdgcn_update_dpp( (int)v, (int)v, 0x104, 0xf, 0x5, false );
}

/* The split field mul: after the column sums, the two lanes of a pair run
   the two halves of the reference carry chain side by side (rather than
   both running all of it), and each returns five limbs (fe5); fe_join5 makes the full
   element when an operation needs it.  The chain of fe_carry_b is two
   interleaved runs, 0->1->2->3->(4) and 4->5->6->7->8->9->(0); in slots
   s0..s5 lane h = 0 holds h0..h4 (s5 = 0) and lane h = 1 holds h4..h9, so
   one instruction stream advances both runs (the widths 26,25,26,25,26
   agree; only the mask of step 4 differs: t4 = (h4 & M26) + h3>>25 on
   h = 0, h8 += h7>>25 on h = 1).  The two cross terms, c4b into limb 5 and
   h9>>25 into limb 0, are swapped with DPP after the run.  Limbs out:
   h = 0 -> (r0, r1, r2, r3, r4), h = 1 -> (r9, r5, r6, r7, r8).  The same
   limbs as fe_carry_b, so the same as the reference's fe_mul. */
struct fe5 { i32 v[5]; };

__device__ __forceinline__ i64 dpp64_from_lo( i64 old, i64 src ) {   /* h = 1 lanes take lane - 4's src */
  u32 lo = (u32)__builtin_amdgcn_update_dpp( (int)(u32)old, (int)(u32)src, 0x114, 0xf, 0xa, false );
  u32 hi = (u32)__builtin_amdgcn_update_dpp( (int)(u32)((u64)old >> 32), (int)(u32)((u64)src >> 32), 0x114, 0xf, 0xa, false );
  return (i64)(((u64)hi << 32) | lo);
}
__device__ __forceinline__ i64 dpp64_from_hi( i64 old, i64 src ) {   /* h = 0 lanes take lane + 4's src */
  u32 lo = (u32)__builtin_amdgcn_update_dpp( (int)(u32)old, (int)(u32)src, 0x104, 0xf, 0x5, false );
  u32 hi = (u32)__builtin_amdgcn_update_dpp( (int)(u32)((u64)old >> 32), (int)(u32)((u64)src >> 32), 0x104, 0xf, 0x5, false );
  return (i64)(((u64)hi << 32) | lo);
}

__device__ __forceinline__ fe5
fe_mul_half5( fe const & F, fe const & G, half_t const & H ) {
  i32 gs[9], g19[10], f2[10];
  _Pragma("unroll") for( int j=0; j<9; j++ ) gs[j] = vsel( H.mH, G.v[j+1], G.v[j] );
  _Pragma("unroll") for( int j=1; j<9; j++ ) g19[j] = wmul( gs[j], 19 );
  g19[9] = vsel( H.mH, G.v[0], wmul( G.v[9], 19 ) );
  _Pragma("unroll") for( int i=1; i<10; i+=2 ) f2[i] = (i32)((u32)F.v[i] << (u32)H.shF);
  i64 a[5];
  _Pragma("unroll") for( int c=0; c<5; c++ ) a[c] = H.bias;
  _Pragma("unroll") for( int i=0; i<10; i++ ) {
    _Pragma("unroll") for( int c=0; c<5; c++ ) {
      int j = 2*c - i;
      i32 g = (j >= 0) ? gs[j] : g19[j + 10];
      i32 f = (i & 1) ? f2[i] : F.v[i];
      a[c] = mac( f, g, a[c] );
    }
  }
  /* a[c] is column 2c (h = 0) or 2c+1 (h = 1), pre-biased */
  i64 s1 = dpp64_from_hi( a[2], a[0] );    /* h1 | h5 */
  i64 s0 = dpp64_from_lo( a[0], a[2] );    /* h0 | h4 */
  i64 s2 = dpp64_from_lo( a[1], a[3] );    /* h2 | h6 */
  i64 s3 = dpp64_from_hi( a[3], a[1] );    /* h3 | h7 */
  i64 s4 = dpp64_from_lo( a[2], a[4] );    /* h4 | h8 */
  i64 s5 = a[4] & H.k5;                    /* 0  | h9 */
  s1 += s0 >> 26;
  s2 += s1 >> 25;
  s3 += s2 >> 26;
  s4 = (s4 & H.m4) + (s3 >> 25);           /* t4 | h8 */
  s5 += s4 >> 26;                          /* c4b | h9 */
  i64 const y = s5 >> H.shz;               /* c4b | h9 >> 25 */
  u32 const ylo = (u32)y, yhi = (u32)((u64)y >> 32);
  u32 zl = (u32)__builtin_amdgcn_update_dpp( (int)ylo, (int)ylo, 0x104, 0xf, 0x5, false );
  zl = (u32)__builtin_amdgcn_update_dpp( (int)zl, (int)ylo, 0x114, 0xf, 0xa, false );
  u32 const zh = (u32)__builtin_amdgcn_update_dpp( (int)yhi, (int)yhi, 0x104, 0xf, 0x5, false );
  i64 const z = (i64)(((u64)zh << 32) | zl);   /* h = 0: h9 >> 25; h = 1: c4b (low word) */
  i64 const t0 = (s0 & ((1L<<26) - 1)) + z * 19;
  i32 const cin = vsel( H.mH, (i32)zl, (i32)(t0 >> 26) );
  u32 const w0 = (u32)vsel( H.mH, (i32)(u32)s5, (i32)(u32)t0 );
  fe5 o;
  o.v[0] = (i32)(w0 & H.mo0) - H.bo0;
  o.v[1] = (i32)((u32)s1 & ((1u<<25) - 1u)) - (1<<24) + cin;
  o.v[2] = (i32)((u32)s2 & ((1u<<26) - 1u)) - (1<<25);
  o.v[3] = (i32)((u32)s3 & ((1u<<25) - 1u)) - (1<<24);
  o.v[4] = (i32)((u32)s4 & ((1u<<26) - 1u)) - (1<<25);
  return o;
}

__device__ __forceinline__ fe fe_join5( fe5 const & o ) {
  fe r;
  r.v[0] = (i32)half_from_lo( (u32)o.v[0] );
  r.v[9] = (i32)half_from_hi( (u32)o.v[0] );
  _Pragma("unroll") for( int k=1; k<5; k++ ) {
    r.v[k]   = (i32)half_from_lo( (u32)o.v[k] );
    r.v[k+4] = (i32)half_from_hi( (u32)o.v[k] );
  }
  return r;
}

__device__ __forceinline__ fe5
quad8_p3_ownc5( fe const & C, half_t const & H ) {
  fe a, b;
  _Pragma("unroll") for( int k=0; k<10; k++ ) { a.v[k] = qp<0,0,2,2>( C.v[k] ); b.v[k] = qp<1,3,1,3>( C.v[k] ); }
  return fe_mul_half5( a, b, H );
}

/* quad8_body_ownc on split limbs: every per-limb step (the operand
   combination, the mix) runs on the lane's five limbs, and the pair joins
   the operand before the mul and the mixed coordinate after it */
__device__ __forceinline__ void
quad8_body_ownc5( fe & C, fe5 const & pm, fe const & qrow, bool isD, bool neg, u64 mD, int qd, half_t const & H ) {
  i32 c1 = (qd == 0) ? 1 : (qd == 1) ? (isD ? 0 : -1) : (isD ? 1 : 0);
  i32 c2 = (qd <= 1 || !isD) ? 1 : 0;
  i32 sh = (qd == 3) ? 1 : 0;
  asm( "" : "+v"(c1), "+v"(c2) );
  fe5 a5;
  _Pragma("unroll") for( int k=0; k<5; k++ )
    a5.v[k] = lin2( c1, qp<2,2,2,0>( pm.v[k] ), c2, qp<1,1,0,3>( pm.v[k] ) );
  fe const a = fe_join5( a5 );
  fe b;
  _Pragma("unroll") for( int k=0; k<10; k++ ) b.v[k] = vsel( mD, (i32)((u32)a.v[k] << sh), qrow.v[k] );
  fe5 const m = fe_mul_half5( a, b, H );
  i32 s0 = neg ? -1 : 1;
  i32 x = isD ? (qd == 1 ? -1 : (qd == 3 ? 0 : 1)) : (qd >= 2 ? 1 : 0);
  i32 y = isD ? ((qd & 1) ? 1 : -1)               : (qd <= 1 ? 2 : (qd == 2 ? -1 : 1));
  i32 z = isD ? (qd == 0 ? 0 : (qd == 2 ? -1 : 1)) : (qd == 0 ? s0 : (qd == 1 ? -s0 : 0));
  asm( "" : "+v"(x), "+v"(y), "+v"(z) );
  fe5 c5;
  _Pragma("unroll") for( int k=0; k<5; k++ )
    c5.v[k] = lin3( x, qp<1,1,0,0>( m.v[k] ), y, qp<2,2,1,1>( m.v[k] ), z, qp<3,3,2,2>( m.v[k] ) );
  C = fe_join5( c5 );
}

/* k_dsm8's body for lane gt of the launch (signature gt >> 3); bi12 filled
   (bi12_fill), evl: 8 event rows of 33 words for the wave's 8 signatures.
   Also the streaming tile's latency chunks (k_tile_persist). */
__device__ __forceinline__ void
dsm8_body( u32 gt, u32 n, i8 * __restrict__ err, u8 * __restrict__ ws, ws_layout_t L, int want_stats,
           i32 (* __restrict__ bi12)[48], u64 (* __restrict__ evl)[33], u64 tc = 0UL ) {
  u32 i = gt >> 3;
  int qd = (int)(threadIdx.x & 3u);
  int hh = (int)((threadIdx.x >> 2) & 1u);            /* which half of every field mul this lane computes */
  bool act = (i < n) && (err[i] == 1);
  if( act && (ws[L.ds + 2u*i] | ws[L.ds + 2u*i + 1u]) ) {            /* A or R undecodable */
    act = false;
    if( qd == 0 && !hh ) err[i] = (i8)-2;
  }
  size_t N = L.N;
  u32 ii = (i < n) ? i : 0u;
  i32 * Ail = (i32 *)(ws + L.Ai) + (size_t)ii*384u;
  u64 const m1 = __builtin_amdgcn_ballot_w64( qd & 1 ), m2 = __builtin_amdgcn_ballot_w64( qd & 2 );
  half_t const H = half_ctx( hh );

  /* -A and its odd multiples (cached rows; lane q writes row q, the h = 0 half) */
  ai_table_quad( act, act && !hh, qd, m1, m2, (i32 const *)(ws + L.A), N, ii, Ail );

  u64 const * dg = (u64 const *)(ws + L.dig) + (size_t)ii*32u;
  int p   = act ? ((int const *)(ws + L.top))[ii] : -1;
  int ph  = act ? (p >= 0 ? PH_DBL : PH_FIN) : PH_DONE;
  evq eva, evb;                                      /* digit events of h and s */
  {
    u64 * row = evl[(threadIdx.x & 63u) >> 3];       /* one row per signature of the wave */
    u32 ne = act ? ((u32 const *)(ws + L.evn))[ii] : 0u;
    u32 wa = ((ne & 0xffu) + 3u) >> 2, wb = (((ne >> 8) & 0xffu) + 3u) >> 2;
    for( u32 k=threadIdx.x & 7u; k<wa; k+=8u ) row[k]       = dg[k];   /* the 8 lanes copy the row together */
    for( u32 k=threadIdx.x & 7u; k<wb; k+=8u ) row[16u + k] = dg[16u + k];
    __syncthreads();
    eva.init( (u16 const *)row,        (int)(ne & 0xffu) );
    evb.init( (u16 const *)(row + 16), (int)((ne >> 8) & 0xffu) );
  }
  i32 const * Rw = (i32 const *)(ws + L.R);
  u32 nha = 0, nhb = 0;
  u32 nit = (u32)(p + 1);
  bool qneg = false;
  fe qrow = fe_zero();
  fe C = (qd == 2) ? fe_zero() : fe_one();   /* identity: own coordinate (Z, T, X, Y)[q] = (1, 1, 0, 1) */
  u32 lvl = 0u;

  for( ;; ) {
    if( tc ) tile_age_prio( tc, lvl );
    fe5 pm5 = quad8_p3_ownc5( C, H );          /* q0 u.Z, q1 u.Y, q2 u.X, q3 u.T (split limbs) */

    bool fin = (ph == PH_FIN);
    /* each lane parks its own p1p1->p3 product in its row of entry 0 of the
       signature's Ai table (no ADD op reads it any more); the compare runs
       once after the loop */
    if( __any( fin ) ) {
      fe const pm = fe_join5( pm5 );           /* all 8 lanes of a signature finish together */
      if( fin ) {
        int4 * d_ = (int4 *)(Ail + qd*12);
        d_[0] = make_int4( pm.v[0], pm.v[1], pm.v[2], pm.v[3] );
        d_[1] = make_int4( pm.v[4], pm.v[5], pm.v[6], pm.v[7] );
        d_[2] = make_int4( pm.v[8], pm.v[9], 0, 0 );
        ph = PH_DONE;
      }
    }
    if( __all( ph == PH_DONE ) ) break;

    bool isD = (ph == PH_DBL);
    u64 mD = __builtin_amdgcn_ballot_w64( isD );
    quad8_body_ownc5( C, pm5, qrow, isD, qneg, mD, qd, H );

    /* the event just executed is consumed; the next op follows from the
       event heads (an event at position p means a digit at p).  Branch-free:
       on one wave per SIMD every exec-mask branch is an issue slot. */
    bool const wasA = ph == PH_ADDA, wasB = ph == PH_ADDB, wasD = ph == PH_DBL;
    eva.j -= (int)wasA; evb.j -= (int)wasB;
    eva.load(); evb.load();
    bool const toA = wasD && eva.pos == p;
    bool const toB = !toA && (wasD || wasA) && evb.pos == p;
    bool const adv = (wasD || wasA || wasB) && !toA && !toB;
    p -= (int)adv;
    ph = toA ? PH_ADDA : toB ? PH_ADDB : adv ? ((p < 0) ? PH_FIN : PH_DBL) : ph;
    nha += (u32)toA; nhb += (u32)toB;

    /* this lane's row of the next op's operand: q0 qP, q1 qM, q2 qZ, q3 qT;
       rows of an entry are [Z, Y-X, Y+X, 2dT], a negative digit swaps Y-X/Y+X
       (loaded by every lane; only an ADD reads it) */
    {
      int const d = toA ? eva.dig : evb.dig;
      int const e = ((d < 0 ? -d : d) >> 1) & 7;
      qneg = d < 0;
      int const row = (qd == 0) ? (qneg ? 1 : 2) : (qd == 1) ? (qneg ? 2 : 1) : (qd == 2) ? 0 : 3;
      int4 const * src = toA ? (int4 const *)(Ail + e*48 + row*12) : (int4 const *)&bi12[e][row*12];
      int4 x0 = src[0], x1 = src[1], x2 = src[2];
      qrow.v[0] = x0.x; qrow.v[1] = x0.y; qrow.v[2] = x0.z; qrow.v[3] = x0.w;
      qrow.v[4] = x1.x; qrow.v[5] = x1.y; qrow.v[6] = x1.z; qrow.v[7] = x1.w;
      qrow.v[8] = x2.x; qrow.v[9] = x2.y;
    }
  }

  /* the limb compare (fd_ed25519_user.c:417-425), once per wave, all lanes
     converged: q0 Z*RX vs X, q1 Z*RY vs Y, quad AND */
  {
    fe pm;
    int4 const * s_ = (int4 const *)(Ail + qd*12);
    int4 x0 = s_[0], x1 = s_[1], x2 = s_[2];
    pm.v[0] = x0.x; pm.v[1] = x0.y; pm.v[2] = x0.z; pm.v[3] = x0.w;
    pm.v[4] = x1.x; pm.v[5] = x1.y; pm.v[6] = x1.z; pm.v[7] = x1.w;
    pm.v[8] = x2.x; pm.v[9] = x2.y;
    _Pragma("unroll") for( int k=0; k<10; k++ ) qrow.v[k] = Rw[(size_t)((qd & 1)*10 + k)*N + ii];
    fe Z, ref;
    _Pragma("unroll") for( int k=0; k<10; k++ ) {
      Z.v[k] = qb<0>( pm.v[k] );
      ref.v[k] = qp<2,1,2,1>( pm.v[k] );    /* q0 <- X (lane 2), q1 <- Y (own) */
    }
    fe xz = fe_mul_fold1( Z, qrow );
    bool eq = true;
    _Pragma("unroll") for( int k=0; k<8; k++ ) eq = eq && (xz.v[k] == ref.v[k]);
    int e01 = (int)eq;
    int both = qb<0>( e01 ) & qb<1>( e01 );
    if( act && qd == 0 && !hh ) err[i] = (i8)(both ? 0 : -3);
  }

  if( want_stats && i < n && qd == 0 && !hh ) {
    u32 * st = (u32 *)(ws + L.st);
    st[i] = act ? nit : 0u; st[N + i] = act ? nha : 0u; st[2*N + i] = act ? nhb : 0u;
  }
}

/* The R' that dsm8_body parked, for a kernel that runs after k_dsm8
   (k_strict).  Both halves (hh = 0, 1) of a signature's 8 lanes join their
   split limbs into the same full product (fe_join5) and store it to the
   same row Ail + qd*12, the same bytes twice: the slab ends up in k_dsm4's
   layout, row 0 = Z, row 1 = Y, row 2 = X. */
__device__ __forceinline__ void
dsm8_load_parked( fe & X, fe & Y, fe & Z, i32 const * __restrict__ Ail ) {
  dsm4_load_parked( X, Y, Z, Ail );
}

__global__ void __launch_bounds__(64)
k_dsm8( u32 n, i8 * __restrict__ err, u8 * __restrict__ ws, ws_layout_t L, int want_stats, i8 * __restrict__ out ) {
  __shared__ __attribute__((aligned(16))) i32 bi12[8][48];
  __shared__ u64 evl[8][33];
  bi12_fill( bi12 );
  __syncthreads();
  u32 const gt = blockIdx.x * 64u + threadIdx.x;
  dsm8_body( gt, n, err, ws, L, want_stats, bi12, evl );
  /* every verdict, straight to mapped host memory, by the lane that wrote it */
  if( out && (gt >> 3) < n && !(threadIdx.x & 7u) ) out[gt >> 3] = err[gt >> 3];
}

#endif /* FD_ED25519_DSM8_H */
