/* firedancer_amd/csrc/fd_ed25519_dsm.h
 *
 * The group ops, vsel, the per-lane step stream (evq) and k_dsm, one lane
 * per signature.  Included by fd_ed25519_dsm4.h (and so by dsm8),
 * fd_ed25519_pool.h and fd_ed25519_tile.h.
 */

#ifndef FD_ED25519_DSM_H
#define FD_ED25519_DSM_H

#include "fd_ed25519_ws.h"

/* ------------------------------------------------------------------ */
/* k_dsm                                                                */

struct p1p1 { fe X, Y, Z, T; };
struct p3   { fe X, Y, Z, T; };

/* p2/p3 doubling, AVX flow (avx/fd_ed25519_ge.c:493-498):
   [(X+Y)^2, Y^2, X^2, 2Z^2] -> [a-b-c, b+c, b-c, d-b+c] */
__device__ __forceinline__ p1p1
ge_dbl( fe const & X, fe const & Y, fe const & Z ) {
  fe a = fe_sqn<1>( fe_add( X, Y ) );
  fe b = fe_sqn<1>( Y );
  fe c = fe_sqn<1>( X );
  fe d = fe_sqn<2>( Z );
  p1p1 t;
  _Pragma("unroll") for( int k=0; k<10; k++ ) {
    t.X.v[k] = a.v[k] - b.v[k] - c.v[k];
    t.Y.v[k] = b.v[k] + c.v[k];
    t.Z.v[k] = b.v[k] - c.v[k];
    t.T.v[k] = d.v[k] - b.v[k] + c.v[k];
  }
  return t;
}

/* p1p1 -> p3, AVX lanes Z=Z*T, Y=Y*Z, X=X*T, T=X*Y (:502-504) */
__device__ __forceinline__ p3
ge_p1p1_to_p3( p1p1 const & t ) {
  p3 u;
  /* operand order chosen so the products share pre-multiples: g in {T, Y}
     (x19) and f in {Z, X} (x2); mul is commutative at the integer level */
  u.Z = fe_mul( t.Z, t.T );
  u.Y = fe_mul( t.Z, t.Y );
  u.X = fe_mul( t.X, t.T );
  u.T = fe_mul( t.X, t.Y );
  return u;
}

/* the same products as interleaved, carry-folded pairs (fe_mul_fold2w) */
__device__ __forceinline__ p3
ge_p1p1_to_p3_fold( p1p1 const & t ) {
  p3 u;
  fe_mul_fold2w( u.Z, t.Z, t.T, u.Y, t.Z, t.Y );
  fe_mul_fold2w( u.X, t.X, t.T, u.T, t.X, t.Y );
  return u;
}

/* the add/sub (and madd/msub when qZ==1) body (:505-518).  qZ_one: the
   table Z lane is 1 (base-point table) so Z*1 is the carry chain. */
template<bool QZ_ONE>
__device__ __forceinline__ p1p1
ge_add( p3 const & u, fe const & qZ, fe const & qYmX, fe const & qYpX, fe const & qT2d, bool neg ) {
  fe ymx = fe_sub( u.Y, u.X ), ypx = fe_add( u.Y, u.X );
  fe ZZ = QZ_ONE ? fe_mul_one( u.Z ) : fe_mul( u.Z, qZ );
  fe MM = fe_mul( ymx, neg ? qYpX : qYmX );
  fe PP = fe_mul( ypx, neg ? qYmX : qYpX );
  fe TT = fe_mul( u.T, qT2d );
  p1p1 t;
  _Pragma("unroll") for( int k=0; k<10; k++ ) {
    i32 z2 = ZZ.v[k] + ZZ.v[k];
    t.X.v[k] = PP.v[k] - MM.v[k];
    t.Y.v[k] = PP.v[k] + MM.v[k];
    i32 zp = z2 + TT.v[k], zm = z2 - TT.v[k];
    t.Z.v[k] = neg ? zm : zp;
    t.T.v[k] = neg ? zp : zm;
  }
  return t;
}

/* p3 -> cached with the AVX "x[1,1,1,2d]" multiply (:440-446, :475-479) */
__device__ __forceinline__ void
ge_to_cached( fe & cZ, fe & cYmX, fe & cYpX, fe & cT2d, p3 const & u ) {
  fe const D2 = {FD_AMD_FE_D2};
  fe Z1 = fe_mul_one( u.Z ), Y1 = fe_mul_one( u.Y ), X1 = fe_mul_one( u.X );
  cT2d = fe_mul( u.T, D2 );
  cZ = Z1; cYmX = fe_sub( Y1, X1 ); cYpX = fe_add( Y1, X1 );
}

/* Base-point table in LDS, rows [Z(=1), Y-X, Y+X, 2dT] x 10 limbs per entry
   (table/fd_ed25519_ge_bi_precomp_avx.c:30-112 lane order). */
__constant__ static i32 const BI_TABLE[8][3][10] = FD_AMD_BI_PRECOMP;   /* rows y+x, y-x, 2dxy */

/* The base-point table in the Ai slab's row layout (rows [Z = 1 | Y-X |
   Y+X | 2dT] x 12 limbs, 10 used): an ADD-A row comes from the signature's
   Ai slab, an ADD-B row from here, with the same three 16-B loads through
   one generic pointer.  Filled by the wave before the DSM bodies run. */
__device__ __forceinline__ void
bi12_fill( i32 (* __restrict__ bi12)[48] ) {
  for( int k=threadIdx.x & 63; k<8*48; k+=64 ) {
    int e = k / 48, c = (k % 48) / 12, l = k % 12;
    i32 v = 0;
    if( l < 10 ) {
      if( c == 0 ) v = (l == 0);
      else if( c == 1 ) v = BI_TABLE[e][1][l];
      else if( c == 2 ) v = BI_TABLE[e][0][l];
      else v = BI_TABLE[e][2][l];
    }
    bi12[e][k % 48] = v;
  }
}

/* Branch-free per-lane select: v_cndmask_b32 on a wave lane mask (ballot).
   Plain ?: on the op-stream selects lets LLVM re-form divergent branches
   around the field muls (both sides then run with copies in between). */
__device__ __forceinline__ i32 vsel( u64 m, i32 t, i32 f ) {
  i32 r;
  asm( "v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(m) );
  return r;
}

enum { PH_DBL = 0, PH_ADDA = 1, PH_ADDB = 2, PH_FIN = 3, PH_DONE = 4 };

/* One scalar's slide-digit events (k_prep), walked from the top.  The
   kernel first copies the signature's event row into LDS, so a pop is one
   ds_read_u16 (an LDS wait, not a memory wait, when it lands in a
   divergent branch). */
struct evq {
  u16 const * e;     /* the list in LDS */
  int j, pos, dig;   /* current event index (descending), its position (-1: none left) and digit */
  __device__ __forceinline__ void load() {
    u32 x = (j >= 0) ? (u32)e[j] : 0xffffu;
    pos = (j >= 0) ? (int)(x & 0xffu) : -1;
    dig = (int)(i8)(x >> 8);
  }
  __device__ __forceinline__ void init( u16 const * e_, int n ) { e = e_; j = n - 1; load(); }
  __device__ __forceinline__ void pop() { j--; load(); }
};

/* k_dsm: [h](-A) + [s]B as a per-lane STEP STREAM.
 *
 * The reference loop (avx/fd_ed25519_ge.c:488-523) is, per bit position p
 * from the top:  DBL ; [ADD Ai[|a_p|/2] if a_p] ; [MADD Bi[|b_p|/2] if b_p] ;
 * with p1p1->p3 before every add and p1p1->p2 before every doubling.
 * p1p1->p2 computes exactly the first three products of p1p1->p3
 * (X*T, Y*Z, Z*T), so every op of the stream has the same shape:
 *
 *     u  = p1p1->p3(t)                        4 field muls
 *     m0..m3 = op-specific 4 field muls        DBL: (X+Y)^2, Y^2, X^2, Z*2Z
 *                                              ADD: Z*qZ, (Y-X)*qM, (Y+X)*qP, T*qT
 *     t  = op-specific linear mix
 *
 * so each lane walks ITS OWN op sequence and every step does 8 useful field
 * muls on every lane (no predicated adds).  Bit-exactness: sq(f) == mul(f,f),
 * sq2(f) == mul(f,f+f) and mul(f,1) == carry(f) at the integer level
 * (SURVEY.md s7 "Measured equivalences"), so a uniform mul is the
 * reference's sq / sq2 / madd Z*1 bit for bit.  A lane whose last op is done
 * takes one more step (PH_FIN): its p1p1->p2 result is R', compared with
 * the limb memcmp of fd_ed25519_user.c:417-425, then it idles (PH_DONE).
 */
/* Streaming tile (k_tile_persist): the wave's issue priority follows the
   age of its chunk, claimed at s_memrealtime tc (100 MHz): 0 below 0.4 ms,
   then one level per 0.4 ms.  Two waves share a SIMD, and at equal priority
   the arbiter prefers the older WAVE -- in a persistent kernel always the
   same one, so one wave of each pair ran its chunks ~1.1 ms and the other
   ~5 ms, and the tile publishes in order behind the slow ones.  By chunk age
   the older CHUNK goes first.  Scalar only (SGPRs, s_setprio). */
__device__ __forceinline__ void
tile_age_prio( u64 tc, u32 & lvl ) {
  u64 const el = __builtin_amdgcn_s_memrealtime() - tc;
  u32 const want = el < 40000UL ? 0u : el < 80000UL ? 1u : el < 120000UL ? 2u : 3u;
  if( want == lvl ) return;
  lvl = want;
  if( want == 1u )      __builtin_amdgcn_s_setprio( 1 );
  else if( want == 2u ) __builtin_amdgcn_s_setprio( 2 );
  else if( want == 3u ) __builtin_amdgcn_s_setprio( 3 );
  else                  __builtin_amdgcn_s_setprio( 0 );
}

__device__ __forceinline__ void
dsm_lane_body( u32 i, u32 n, i8 * __restrict__ err, u8 * __restrict__ ws, ws_layout_t L, int want_stats,
               i32 (* __restrict__ bi)[48], u64 (* __restrict__ evl)[33], u64 tc = 0UL ) {
  /* bi: the base-point table in the Ai slab's row layout (bi12_fill), so
     ADD-A and ADD-B operands load alike */
  bool act = (i < n) && (err[i] == 1);
  if( act && (ws[L.ds + 2u*i] | ws[L.ds + 2u*i + 1u]) ) { err[i] = (i8)-2; act = false; }   /* A or R undecodable */
  size_t N = L.N;
  u32 ii = (i < n) ? i : 0u;
  i32 * Ail = (i32 *)(ws + L.Ai) + (size_t)ii*384u;   /* this lane's 8 x 4 x 12 table */

  /* -A (p3, Z = 1) and its odd multiples Ai (:423-481) -> HBM */
  {
    p3 A;
    i32 const * Aw = (i32 const *)(ws + L.A);
    _Pragma("unroll") for( int k=0; k<10; k++ ) {
      A.X.v[k] = act ? Aw[(size_t)(k   )*N + ii] : 0;
      A.Y.v[k] = act ? Aw[(size_t)(10+k)*N + ii] : (k==0);
      A.T.v[k] = act ? Aw[(size_t)(20+k)*N + ii] : 0;
      A.Z.v[k] = (k==0);
    }
    fe cZ, cYmX, cYpX, cT2d;
    ge_to_cached( cZ, cYmX, cYpX, cT2d, A );
#   define AI_ROW( e, r, f ) do {                                                   \
      int4 * d_ = (int4 *)(Ail + (e)*48 + (r)*12);                                  \
      d_[0] = make_int4( f.v[0], f.v[1], f.v[2], f.v[3] );                          \
      d_[1] = make_int4( f.v[4], f.v[5], f.v[6], f.v[7] );                          \
      d_[2] = make_int4( f.v[8], f.v[9], 0, 0 );                                    \
    } while(0)
#   define AI_STORE( e ) do { AI_ROW( e, 0, cZ ); AI_ROW( e, 1, cYmX ); AI_ROW( e, 2, cYpX ); AI_ROW( e, 3, cT2d ); } while(0)
    if( act ) AI_STORE( 0 );
    p1p1 t = ge_dbl( A.X, A.Y, A.Z );
    p3 A2 = ge_p1p1_to_p3( t );
    for( int e=0; e<7; e++ ) {
      p1p1 s2 = ge_add<false>( A2, cZ, cYmX, cYpX, cT2d, false );
      p3 u = ge_p1p1_to_p3( s2 );
      ge_to_cached( cZ, cYmX, cYpX, cT2d, u );
      if( act ) AI_STORE( e+1 );
    }
#   undef AI_STORE
#   undef AI_ROW
  }

  /* lane state */
  u64 const * dg = (u64 const *)(ws + L.dig) + (size_t)ii*32u;
  int p   = act ? ((int const *)(ws + L.top))[ii] : -1;
  int ph  = act ? (p >= 0 ? PH_DBL : PH_FIN) : PH_DONE;
  evq eva, evb;                                      /* digit events of h and s */
  {
    u64 * row = evl[threadIdx.x];                    /* this wave's event rows (33: bank spread) */
    u32 ne = act ? ((u32 const *)(ws + L.evn))[ii] : 0u;
    u32 wa = ((ne & 0xffu) + 3u) >> 2, wb = (((ne >> 8) & 0xffu) + 3u) >> 2;
    for( u32 k=0; k<wa; k++ ) row[k]       = dg[k];
    for( u32 k=0; k<wb; k++ ) row[16u + k] = dg[16u + k];
    eva.init( (u16 const *)row,        (int)(ne & 0xffu) );
    evb.init( (u16 const *)(row + 16), (int)((ne >> 8) & 0xffu) );
  }
  i32 const * Rw = (i32 const *)(ws + L.R);
  u32 nha = 0, nhb = 0;
  u32 nit = (u32)(p + 1);
  bool qneg = false;

  /* the next op's table operand q = [qZ | qM | qP | qT] (40 limbs) */
  fe q[4];
  _Pragma("unroll") for( int r=0; r<4; r++ ) q[r] = fe_zero();
# define QV( R_, K_ ) q[R_].v[K_]
# define Q_SET( R_, K_, V_ ) ( q[R_].v[K_] = (V_) )
  p1p1 t;   /* identity as a completed point: p1p1->p3 gives (0,1,1,0) */
  t.X = fe_zero(); t.Y = fe_one(); t.Z = fe_one(); t.T = fe_one();
  u32 lvl = 0u;

  for( ;; ) {
    if( tc ) tile_age_prio( tc, lvl );
    /* p1p1 -> p3 (its X,Y,Z are the reference's p1p1 -> p2) */
    p3 u = ge_p1p1_to_p3_fold( t );

    bool fin = (ph == PH_FIN);
    /* R' = u's (X, Y, Z) parks in the lane's own Ai rows (no ADD op reads
       them any more); the compare runs once for the whole wave after the
       loop instead of once per distinct finishing step */
    if( __any( fin ) ) {
      if( fin ) {
        int4 * d_ = (int4 *)Ail;
        d_[0] = make_int4( u.X.v[0], u.X.v[1], u.X.v[2], u.X.v[3] );
        d_[1] = make_int4( u.X.v[4], u.X.v[5], u.X.v[6], u.X.v[7] );
        d_[2] = make_int4( u.X.v[8], u.X.v[9], u.Y.v[0], u.Y.v[1] );
        d_[3] = make_int4( u.Y.v[2], u.Y.v[3], u.Y.v[4], u.Y.v[5] );
        d_[4] = make_int4( u.Y.v[6], u.Y.v[7], u.Y.v[8], u.Y.v[9] );
        d_[5] = make_int4( u.Z.v[0], u.Z.v[1], u.Z.v[2], u.Z.v[3] );
        d_[6] = make_int4( u.Z.v[4], u.Z.v[5], u.Z.v[6], u.Z.v[7] );
        d_[7] = make_int4( u.Z.v[8], u.Z.v[9], 0, 0 );
        ph = PH_DONE;
      }
    }
    if( __all( ph == PH_DONE ) ) break;

    /* op body: 4 field muls with per-lane operands, paired so that DBL and
       ADD share what they can: m0 = (X+Y)*[(X+Y) | qP], m1 = [Y | Y-X]*[Y | qM],
       m2 = [X | Z]*[X | qZ], m3 = [Z | T]*[2Z | qT] */
    bool isD = (ph == PH_DBL);
    u64 mD = __builtin_amdgcn_ballot_w64( isD ), mN = __builtin_amdgcn_ballot_w64( qneg );
    fe m0, m1, m2, m3;
    {
      fe a0, b0, a1, b1, a2, b2, a3, b3;
      _Pragma("unroll") for( int k=0; k<10; k++ ) {
        i32 xy = u.X.v[k] + u.Y.v[k];
        a0.v[k] = xy;                                     b0.v[k] = vsel( mD, xy, QV( 2, k ) );
        a1.v[k] = vsel( mD, u.Y.v[k], u.Y.v[k] - u.X.v[k] ); b1.v[k] = vsel( mD, u.Y.v[k], QV( 1, k ) );
        /* DBL Z*2Z pairs with ADD Z*qZ (shared a = Z), DBL X^2 with ADD T*qT */
        a2.v[k] = u.Z.v[k];                              b2.v[k] = vsel( mD, u.Z.v[k] + u.Z.v[k], QV( 0, k ) );
        a3.v[k] = vsel( mD, u.X.v[k], u.T.v[k] );        b3.v[k] = vsel( mD, u.X.v[k], QV( 3, k ) );
      }
      /* m0, m1, m3 come back with their limbs' rounding offsets b (2^25
         even, 2^24 odd) still added: the mix below folds them into its
         own adds; m2 is exact */
      fe_mul_fold2w<true, true>( m0, a0, b0, m1, a1, b1 );
      fe_mul_fold2w<false, true>( m2, a2, b2, m3, a3, b3 );
    }
    /* lanes that are done (PH_DONE) keep computing on don't-care values:
       nothing they compute is stored.
       DBL mix [a-b-c, b+c, b-c, d-b+c] with a=m0 b=m1 c=m3 d=m2 (m2 = Z*2Z, m3 = X^2);
       ADD mix [P-M, P+M, 2Z+sT, 2Z-sT] with P=m0 M=m1 Z=m2 T=m3, s = neg ? -1 : 1.
       With sA3 = s'*m3 (s' = -1 on DBL lanes, one v_xad_u32), 11 ops per limb:
         X = (m0 - m1) + (sA3 & D)            Y = m1 + (D ? m3 : m0)
         Z = (D ? m1 : 2 m2) + sA3            T = (m2 << (D ? 0 : 2)) - Z
       plus per-lane offset corrections cX (DBL: +b), cZ (ADD: -s b) and the
       uniform -2b of Y, each folded into a v_add3_u32.  Limbs equal the
       reference's wrapping int32 adds (every identity holds mod 2^32). */
    {
      u64 mS = mD | mN;
      i32 Dv = vsel( mD, -1, 0 ), Sv = vsel( mS, -1, 0 ), Sn = vsel( mS, 1, 0 );
      i32 cXe = Dv & (1<<25), cXo = Dv & (1<<24);
      i32 cZe = vsel( mD, 0, vsel( mN, (1<<25), -(1<<25) ) ), cZo = vsel( mD, 0, vsel( mN, (1<<24), -(1<<24) ) );
      i32 const nb2e = (i32)fd_opaque( -(2L<<25) ), nb2o = (i32)fd_opaque( -(2L<<24) );   /* SGPR */
      i32 const sT = vsel( mD, 0, 2 );                     /* T = (m2 << sT) - Z: DBL m2 - Z, ADD 4 m2 - Z */
      _Pragma("unroll") for( int k=0; k<10; k++ ) {
        i32 cX = (k & 1) ? cXo : cXe, cZ = (k & 1) ? cZo : cZe;
        i32 A0 = m0.v[k], A1 = m1.v[k], A2 = m2.v[k], A3 = m3.v[k];
        i32 sA3 = fd_xad( A3, Sv, Sn );
        i32 z2 = A2 + A2;
        i32 Z = fd_add3( vsel( mD, A1, z2 ), sA3, cZ );
        t.X.v[k] = fd_add3( A0 - A1, sA3 & Dv, cX );
        t.Y.v[k] = fd_add3s( A1, vsel( mD, A3, A0 ), (k & 1) ? nb2o : nb2e );
        t.Z.v[k] = Z;
        t.T.v[k] = (i32)((u32)A2 << (u32)sT) - Z;
      }
    }

    /* advance the lane's op stream: the event just executed is consumed; the next op follows from the
       event heads (an event at position p means a digit at p) */
    bool const wasA = ph == PH_ADDA, wasB = ph == PH_ADDB, wasD = ph == PH_DBL;
    eva.j -= (int)wasA; evb.j -= (int)wasB;
    eva.load(); evb.load();
    bool const toA = wasD && eva.pos == p;
    bool const toB = !toA && (wasD || wasA) && evb.pos == p;
    bool const adv = (wasD || wasA || wasB) && !toA && !toB;
    p -= (int)adv;
    ph = toA ? PH_ADDA : toB ? PH_ADDB : adv ? ((p < 0) ? PH_FIN : PH_DBL) : ph;
    nha += (u32)toA; nhb += (u32)toB;

    /* stage the next op's operand into q (consumed after the next
       p1p1->p3, so the load latency hides under 4 field muls); every lane
       loads, only an ADD reads it; ADD-A from the Ai slab, ADD-B from the
       LDS table, through one generic pointer (no branch) */
    {
      int const d = toA ? eva.dig : evb.dig;
      int const e = ((d < 0 ? -d : d) >> 1) & 7;
      qneg = d < 0;
      int4 const * src = toA ? (int4 const *)(Ail + e*48) : (int4 const *)&bi[e][0];
      int rowM = qneg ? 2 : 1, rowP = qneg ? 1 : 2;
#     define Q_ROW( r, c ) do {                                                      \
        int4 x0 = src[3*(c)], x1 = src[3*(c)+1], x2 = src[3*(c)+2];                \
        Q_SET( r, 0, x0.x ); Q_SET( r, 1, x0.y ); Q_SET( r, 2, x0.z ); Q_SET( r, 3, x0.w ); \
        Q_SET( r, 4, x1.x ); Q_SET( r, 5, x1.y ); Q_SET( r, 6, x1.z ); Q_SET( r, 7, x1.w ); \
        Q_SET( r, 8, x2.x ); Q_SET( r, 9, x2.y );                                  \
      } while(0)
      Q_ROW( 0, 0 ); Q_ROW( 1, rowM ); Q_ROW( 2, rowP ); Q_ROW( 3, 3 );
#     undef Q_ROW
    }
  }
# undef QV
# undef Q_SET

  /* the limb compare of fd_ed25519_user.c:417-425, once per wave */
  if( act ) {
    int4 const * s_ = (int4 const *)Ail;
    int4 w0 = s_[0], w1 = s_[1], w2 = s_[2], w3 = s_[3], w4 = s_[4], w5 = s_[5], w6 = s_[6], w7 = s_[7];
    fe X = {{ w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y }};
    fe Y = {{ w2.z, w2.w, w3.x, w3.y, w3.z, w3.w, w4.x, w4.y, w4.z, w4.w }};
    fe Z = {{ w5.x, w5.y, w5.z, w5.w, w6.x, w6.y, w6.z, w6.w, w7.x, w7.y }};
    fe RX, RY;
    _Pragma("unroll") for( int k=0; k<10; k++ ) { RX.v[k] = Rw[(size_t)k*N + ii]; RY.v[k] = Rw[(size_t)(10+k)*N + ii]; }
    fe xZ, yZ;
    fe_mul_fold2w( xZ, Z, RX, yZ, Z, RY );
    bool eq = true;
    _Pragma("unroll") for( int k=0; k<8; k++ ) eq = eq && (xZ.v[k] == X.v[k]) && (yZ.v[k] == Y.v[k]);
    err[i] = (i8)(eq ? 0 : -3);
  }
  if( want_stats && i < n ) {
    u32 * st = (u32 *)(ws + L.st);
    st[i] = act ? nit : 0u; st[N + i] = act ? nha : 0u; st[2*N + i] = act ? nhb : 0u;
  }
}

/* The R' = (X, Y, Z) that dsm_lane_body parked in a signature's Ai slab
   (ints 0 / 10 / 20, the int4 stores at its PH_FIN step), for a kernel that
   runs after k_dsm (k_strict).  Only slabs of signatures that were active
   in the loop hold one. */
__device__ __forceinline__ void
dsm_load_parked( fe & X, fe & Y, fe & Z, i32 const * __restrict__ Ail ) {
  int4 const * s_ = (int4 const *)Ail;
  int4 w0 = s_[0], w1 = s_[1], w2 = s_[2], w3 = s_[3], w4 = s_[4], w5 = s_[5], w6 = s_[6], w7 = s_[7];
  X = fe{{ w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y }};
  Y = fe{{ w2.z, w2.w, w3.x, w3.y, w3.z, w3.w, w4.x, w4.y, w4.z, w4.w }};
  Z = fe{{ w5.x, w5.y, w5.z, w5.w, w6.x, w6.y, w6.z, w6.w, w7.x, w7.y }};
}

__global__ void __launch_bounds__(64)
k_dsm( u32 n, i8 * __restrict__ err, u8 * __restrict__ ws, ws_layout_t L, int want_stats ) {
  __shared__ __attribute__((aligned(16))) i32 bi[8][48];
  __shared__ u64 evl[64][33];
  bi12_fill( bi );
  __syncthreads();
  dsm_lane_body( blockIdx.x * 64u + threadIdx.x, n, err, ws, L, want_stats, bi, evl );
}

#endif /* FD_ED25519_DSM_H */
