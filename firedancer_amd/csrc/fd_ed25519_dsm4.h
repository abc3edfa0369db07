/* firedancer_amd/csrc/fd_ed25519_dsm4.h
 *
 * The DPP quad helpers, the quad Ai table and k_dsm4, four lanes per
 * signature.  Included by fd_ed25519_dsm8.h (which runs the same quad flow
 * on two quads) and fd_ed25519_tile.h.
 */

#ifndef FD_ED25519_DSM4_H
#define FD_ED25519_DSM4_H

#include "fd_ed25519_dsm.h"

/* ------------------------------------------------------------------ */
/* k_dsm4: the same op stream with FOUR lanes per signature (16 signatures
 * per wave), for latency: a small batch leaves most SIMDs idle and the
 * verify time is one lane's sequential op stream.  Every step of the op
 * stream is 4 independent field muls (p1p1->p3) followed by 4 independent
 * muls (the op body); lane q of a quad does the q-th mul of each group and
 * the quad exchanges results with DPP quad_perm broadcasts (the AVX build's
 * 4-lane split of fd_ed25519_ge.c:408-527, mapped to a lane quad instead of
 * a ymm register).  The linear mixes are recomputed by all four lanes, so
 * every lane holds the full point between the two mul groups.  Same field
 * ops in the same order as k_dsm: identical limbs.
 *
 *   p1p1->p3 : q0 Z*T -> u.Z   q1 Z*Y -> u.Y   q2 X*T -> u.X   q3 X*Y -> u.T
 *   DBL body : q0 (X+Y)^2      q1 Y^2          q2 X^2          q3 Z*2Z
 *   ADD body : q0 (Y+X)*qP     q1 (Y-X)*qM     q2 Z*qZ         q3 T*qT
 *   FIN      : q0 Z*RX         q1 Z*RY  (then the limb compare, quad AND)
 * Each lane loads only the table row its mul needs (qP/qM/qZ/qT).
 */
template<int K>
__device__ __forceinline__ i32 qb( i32 v ) {   /* broadcast lane K of each quad: DPP quad_perm(K,K,K,K) */
  return __builtin_amdgcn_mov_dpp( v, K * 0x55, 0xf, 0xf, false );
}
__device__ __forceinline__ void qgather( fe const & mine, fe & f0, fe & f1, fe & f2, fe & f3 ) {
  _Pragma("unroll") for( int k=0; k<10; k++ ) {
    f0.v[k] = qb<0>( mine.v[k] ); f1.v[k] = qb<1>( mine.v[k] );
    f2.v[k] = qb<2>( mine.v[k] ); f3.v[k] = qb<3>( mine.v[k] );
  }
}
/* per-lane choice among four values by quad position (lane masks m1,m2:
   bit 0 / bit 1 of q) */
__device__ __forceinline__ i32 q4( u64 m1, u64 m2, i32 a0, i32 a1, i32 a2, i32 a3 ) {
  return vsel( m2, vsel( m1, a3, a2 ), vsel( m1, a1, a0 ) );
}

/* p1p1 -> p3 on a quad: every lane ends with the full u */
__device__ __forceinline__ void
quad_p3( p3 & u, p1p1 const & t, u64 m1, u64 m2 ) {
  fe a, b;
  _Pragma("unroll") for( int k=0; k<10; k++ ) {
    a.v[k] = vsel( m2, t.X.v[k], t.Z.v[k] );                               /* Z Z X X */
    b.v[k] = vsel( m1, t.Y.v[k], t.T.v[k] );                               /* T Y T Y */
  }
  fe pm = fe_mul( a, b );
  qgather( pm, u.Z, u.Y, u.X, u.T );
}

/* DPP quad_perm with a per-destination source lane: lane q reads lane s_q */
template<int S0, int S1, int S2, int S3>
__device__ __forceinline__ i32 qp( i32 v ) {
  return __builtin_amdgcn_mov_dpp( v, S0 | (S1 << 2) | (S2 << 4) | (S3 << 6), 0xf, 0xf, false );
}

/* Own-coordinate form of the step: after the body mul,
   lane q computes only the ONE p1p1 coordinate C = (Z, T, X, Y)[q] that it
   owns, as x*A + y*B + z*D over three DPP-read products with per-lane
   coefficients in {-1,0,1,2} (three v_mad_i64_i32, low 32 bits = the
   reference's wrapping limb adds), instead of every lane mixing all four
   coordinates.  The next p1p1->p3 then reads its operands a = (Z,Z,X,X)[q],
   b = (T,Y,T,Y)[q] with two quad_perm DPP reads per limb.
     DBL  Z = m1-m2   T = m3-m1+m2   X = m0-m1-m2   Y = m1+m2
     ADD  Z = 2m2+-m3 T = 2m2-+m3    X = m0-m1      Y = m0+m1
   A/B/D sources: q0,q1 <- m1,m2,m3; q2,q3 <- m0,m1,m2. */
__device__ __forceinline__ fe
quad_p3_ownc( fe const & C ) {
  fe a, b;
  _Pragma("unroll") for( int k=0; k<10; k++ ) { a.v[k] = qp<0,0,2,2>( C.v[k] ); b.v[k] = qp<1,3,1,3>( C.v[k] ); }
  return fe_mul_fold1( a, b );
}

__device__ __forceinline__ i32
lin3( i32 x, i32 A, i32 y, i32 B, i32 z, i32 D ) {
  i64 acc = fd_pin( (i64)x * (i64)A );
  acc = fd_pin( (i64)y * (i64)B + acc );
  acc = fd_pin( (i64)z * (i64)D + acc );
  return (i32)acc;
}

__device__ __forceinline__ i32
lin2( i32 x, i32 A, i32 y, i32 B ) {
  i64 acc = fd_pin( (i64)x * (i64)A );
  acc = fd_pin( (i64)y * (i64)B + acc );
  return (i32)acc;
}

__device__ __forceinline__ void
quad_body_ownc( fe & C, fe const & pm, fe const & qrow, bool isD, bool neg, u64 mD, int qd ) {
  /* operand a = c1*P1 + c2*P2 with P1 = quad_perm(2,2,2,0) -> X X X Z and
     P2 = quad_perm(1,1,0,3) -> Y Y Z T:  DBL a = [X+Y, Y, X, Z],
     ADD a = [X+Y, Y-X, Z, T];  b = DBL ? a << (q==3) : qrow */
  i32 c1 = (qd == 0) ? 1 : (qd == 1) ? (isD ? 0 : -1) : (isD ? 1 : 0);
  i32 c2 = (qd <= 1 || !isD) ? 1 : 0;
  i32 sh = (qd == 3) ? 1 : 0;
  asm( "" : "+v"(c1), "+v"(c2) );
  fe a, b;
  _Pragma("unroll") for( int k=0; k<10; k++ ) {
    i32 av = lin2( c1, qp<2,2,2,0>( pm.v[k] ), c2, qp<1,1,0,3>( pm.v[k] ) );
    a.v[k] = av;
    b.v[k] = vsel( mD, (i32)((u32)av << sh), qrow.v[k] );
  }
  fe m = fe_mul_fold1( a, b );
  i32 s0 = neg ? -1 : 1;
  i32 x = isD ? (qd == 1 ? -1 : (qd == 3 ? 0 : 1)) : (qd >= 2 ? 1 : 0);
  i32 y = isD ? ((qd & 1) ? 1 : -1)               : (qd <= 1 ? 2 : (qd == 2 ? -1 : 1));
  i32 z = isD ? (qd == 0 ? 0 : (qd == 2 ? -1 : 1)) : (qd == 0 ? s0 : (qd == 1 ? -s0 : 0));
  asm( "" : "+v"(x), "+v"(y), "+v"(z) );   /* opaque: keep full v_mad_i64_i32 (no small-range rewrites) */
  _Pragma("unroll") for( int k=0; k<10; k++ )
    C.v[k] = lin3( x, qp<1,1,0,0>( m.v[k] ), y, qp<2,2,1,1>( m.v[k] ), z, qp<3,3,2,2>( m.v[k] ) );
}

/* op body + mix on a quad.  qrow: this lane's table row (ADD); isD/neg per
   lane (uniform within the quad). */
__device__ __forceinline__ void
quad_body( p1p1 & t, p3 const & u, fe const & qrow, u64 mD, u64 mN, u64 m1, u64 m2 ) {
  fe a, b;
  _Pragma("unroll") for( int k=0; k<10; k++ ) {
    i32 X = u.X.v[k], Y = u.Y.v[k], Z = u.Z.v[k], T = u.T.v[k];
    i32 xy = X + Y;
    i32 aD = q4( m1, m2, xy, Y, X, Z );
    i32 bD = q4( m1, m2, xy, Y, X, Z + Z );
    i32 aA = q4( m1, m2, xy, Y - X, Z, T );
    a.v[k] = vsel( mD, aD, aA );
    b.v[k] = vsel( mD, bD, qrow.v[k] );
  }
  fe m = fe_mul( a, b );
  fe M0, M1, M2, M3;
  qgather( m, M0, M1, M2, M3 );
  _Pragma("unroll") for( int k=0; k<10; k++ ) {
    i32 A0 = M0.v[k], A1 = M1.v[k], A2 = M2.v[k], A3 = M3.v[k];
    i32 z2 = A2 + A2;
    i32 dX = A0 - A1 - A2, dY = A1 + A2, dZ = A1 - A2, dT = A3 - A1 + A2;
    i32 aX = A0 - A1,      aY = A0 + A1;
    i32 zp = z2 + A3, zm = z2 - A3;
    i32 aZ = vsel( mN, zm, zp ), aT = vsel( mN, zp, zm );
    t.X.v[k] = vsel( mD, dX, aX );
    t.Y.v[k] = vsel( mD, dY, aY );
    t.Z.v[k] = vsel( mD, dZ, aZ );
    t.T.v[k] = vsel( mD, dT, aT );
  }
}

/* p3 -> this lane's cached row (q0 Z*1, q1 Y1-X1, q2 Y1+X1, q3 T*2d) */
__device__ __forceinline__ fe
quad_cached_row( p3 const & u, u64 m1, u64 m2 ) {
  fe const D2 = {FD_AMD_FE_D2};
  fe Z1 = fe_mul_one( u.Z ), Y1 = fe_mul_one( u.Y ), X1 = fe_mul_one( u.X );
  fe T2 = fe_mul( u.T, D2 );
  fe r;
  _Pragma("unroll") for( int k=0; k<10; k++ ) r.v[k] = q4( m1, m2, Z1.v[k], Y1.v[k] - X1.v[k], Y1.v[k] + X1.v[k], T2.v[k] );
  return r;
}

/* -A and its odd multiples as cached rows on a quad (k_dsm4, k_dsm8):
   lane q computes row q ([Z, Y-X, Y+X, 2dT]) of every entry and,
   when wr, writes it to the signature's Ai slab Ail; the same ops as
   ge_to_cached / ge_dbl / ge_add (k_ai), so the same limbs. */
__device__ __forceinline__ void
ai_table_quad( bool act, bool wr, int qd, u64 m1, u64 m2, i32 const * __restrict__ Aw, size_t N, u32 ii,
               i32 * __restrict__ Ail ) {
  p3 A;
  _Pragma("unroll") for( int k=0; k<10; k++ ) {
    A.X.v[k] = act ? Aw[(size_t)(k   )*N + ii] : 0;
    A.Y.v[k] = act ? Aw[(size_t)(10+k)*N + ii] : (k==0);
    A.T.v[k] = act ? Aw[(size_t)(20+k)*N + ii] : 0;
    A.Z.v[k] = (k==0);
  }
  fe row = quad_cached_row( A, m1, m2 );
# define AI_ROW4( e ) do {                                                          \
    int4 * d_ = (int4 *)(Ail + (e)*48 + qd*12);                                     \
    d_[0] = make_int4( row.v[0], row.v[1], row.v[2], row.v[3] );                   \
    d_[1] = make_int4( row.v[4], row.v[5], row.v[6], row.v[7] );                   \
    d_[2] = make_int4( row.v[8], row.v[9], 0, 0 );                                 \
  } while(0)
  if( wr ) AI_ROW4( 0 );
  u64 const all = ~0UL, none = 0UL;
  p1p1 t; fe z0 = fe_zero();
  quad_body( t, A, z0, all, none, m1, m2 );            /* DBL(A) */
  p3 A2; quad_p3( A2, t, m1, m2 );
  for( int e=0; e<7; e++ ) {
    fe R0, R1, R2, R3;
    qgather( row, R0, R1, R2, R3 );                    /* rows Z, Y-X, Y+X, 2dT of entry e */
    fe br;
    _Pragma("unroll") for( int k=0; k<10; k++ ) br.v[k] = q4( m1, m2, R2.v[k], R1.v[k], R0.v[k], R3.v[k] );
    quad_body( t, A2, br, none, none, m1, m2 );        /* A2 + Ai[e] */
    p3 u; quad_p3( u, t, m1, m2 );
    row = quad_cached_row( u, m1, m2 );
    if( wr ) AI_ROW4( e+1 );
  }
# undef AI_ROW4
}

/* k_dsm4's body for lane gt of the launch (signature gt >> 2); bi12 filled
   (bi12_fill), evl: 16 event rows of 33 words for the wave's 16 signatures.
   Also the streaming tile's quad chunks (k_tile_persist). */
__device__ __forceinline__ void
dsm4_body( u32 gt, u32 n, i8 * __restrict__ err, u8 * __restrict__ ws, ws_layout_t L, int want_stats,
           i32 (* __restrict__ bi12)[48], u64 (* __restrict__ evl)[33], u64 tc = 0UL ) {
  u32 i = gt >> 2;
  int qd = (int)(threadIdx.x & 3u);
  bool act = (i < n) && (err[i] == 1);
  if( act && (ws[L.ds + 2u*i] | ws[L.ds + 2u*i + 1u]) ) {            /* A or R undecodable */
    act = false;
    if( qd == 0 ) err[i] = (i8)-2;
  }
  size_t N = L.N;
  u32 ii = (i < n) ? i : 0u;
  i32 * Ail = (i32 *)(ws + L.Ai) + (size_t)ii*384u;
  u64 const m1 = __builtin_amdgcn_ballot_w64( qd & 1 ), m2 = __builtin_amdgcn_ballot_w64( qd & 2 );

  /* -A and its odd multiples (cached rows; lane q writes row q) */
  ai_table_quad( act, act, qd, m1, m2, (i32 const *)(ws + L.A), N, ii, Ail );

  u64 const * dg = (u64 const *)(ws + L.dig) + (size_t)ii*32u;
  int p   = act ? ((int const *)(ws + L.top))[ii] : -1;
  int ph  = act ? (p >= 0 ? PH_DBL : PH_FIN) : PH_DONE;
  evq eva, evb;                                      /* digit events of h and s */
  {
    u64 * row = evl[(threadIdx.x & 63u) >> 2];       /* one row per signature of the wave */
    u32 ne = act ? ((u32 const *)(ws + L.evn))[ii] : 0u;
    u32 wa = ((ne & 0xffu) + 3u) >> 2, wb = (((ne >> 8) & 0xffu) + 3u) >> 2;
    for( u32 k=(u32)qd; k<wa; k+=4u ) row[k]       = dg[k];        /* the quad copies the row together */
    for( u32 k=(u32)qd; k<wb; k+=4u ) row[16u + k] = dg[16u + k];
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
    fe pm = quad_p3_ownc( C );              /* q0 u.Z, q1 u.Y, q2 u.X, q3 u.T */

    bool fin = (ph == PH_FIN);
    /* each lane parks its own p1p1->p3 product in its row of entry 0 of the
       signature's Ai table (no ADD op reads it any more); the compare runs
       once after the loop */
    if( __any( fin ) ) {
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
    quad_body_ownc( C, pm, qrow, isD, qneg, mD, qd );

    /* the event just executed is consumed; the next op follows from the
       event heads (an event at position p means a digit at p) */
    /* branch-free, as in k_dsm8 */
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
       rows of an entry are [Z, Y-X, Y+X, 2dT], a negative digit swaps Y-X/Y+X */
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
    if( act && qd == 0 ) err[i] = (i8)(both ? 0 : -3);
  }

  if( want_stats && i < n && qd == 0 ) {
    u32 * st = (u32 *)(ws + L.st);
    st[i] = act ? nit : 0u; st[N + i] = act ? nha : 0u; st[2*N + i] = act ? nhb : 0u;
  }
}

/* One 12-int row of an Ai slab (10 limbs used). */
__device__ __forceinline__ fe
ai_row_load( i32 const * __restrict__ row ) {
  int4 const * s_ = (int4 const *)row;
  int4 x0 = s_[0], x1 = s_[1], x2 = s_[2];
  return fe{{ x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w, x2.x, x2.y }};
}

/* The R' that dsm4_body parked in a signature's Ai slab, for a kernel that
   runs after k_dsm4 (k_strict): lane q of the quad stored its own p1p1->p3
   product in row q of entry 0, so row 0 = Z, row 1 = Y, row 2 = X (row 3 =
   T).  Only slabs of signatures that were active in the loop hold one. */
__device__ __forceinline__ void
dsm4_load_parked( fe & X, fe & Y, fe & Z, i32 const * __restrict__ Ail ) {
  Z = ai_row_load( Ail ); Y = ai_row_load( Ail + 12 ); X = ai_row_load( Ail + 24 );
}

__global__ void __launch_bounds__(64)
k_dsm4( u32 n, i8 * __restrict__ err, u8 * __restrict__ ws, ws_layout_t L, int want_stats, i8 * __restrict__ out ) {
  __shared__ __attribute__((aligned(16))) i32 bi12[8][48];   /* the base-point table in the Ai slab's row layout */
  __shared__ u64 evl[16][33];
  bi12_fill( bi12 );
  __syncthreads();
  u32 const gt = blockIdx.x * 64u + threadIdx.x;
  dsm4_body( gt, n, err, ws, L, want_stats, bi12, evl );
  /* every verdict, straight to mapped host memory, by the lane that wrote it */
  if( out && (gt >> 2) < n && !(threadIdx.x & 3u) ) out[gt >> 2] = err[gt >> 2];
}

#endif /* FD_ED25519_DSM4_H */
