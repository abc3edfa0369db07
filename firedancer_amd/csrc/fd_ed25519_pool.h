/* firedancer_amd/csrc/fd_ed25519_pool.h
 *
 * The pooled DSM for large batches, k_ai -> k_dsmp -> k_fin, with its
 * FD_AMD_DIAG counters.  Only the launch code in fd_ed25519_kernels.hip
 * includes it.
 */

#ifndef FD_ED25519_POOL_H
#define FD_ED25519_POOL_H

#include "fd_ed25519_dsm.h"

/* ------------------------------------------------------------------ */
/* Pooled DSM for large batches: k_ai -> k_dsmp -> k_fin.
 *
 * k_dsm runs every op of a signature's stream (DBL / ADD-A / ADD-B, see
 * above) as the same 8-mul step, so a lane that doubles while its
 * neighbours add still computes general products: each step pays for
 * p1p1->p3 (4 muls) + 4 general muls + per-lane operand selects.  In the
 * reference's own flow (avx/fd_ed25519_ge.c:488-523) a doubling costs
 * p1p1->p2 (3 muls) + 4 squares (55 products each, not 100), and DBLs are
 * about three quarters of the stream.  k_dsmp keeps a POOL of FD_POOL_P
 * signatures per wave in LDS (their p1p1 state and op-stream cursor) and,
 * every step, runs 64 of them that want the SAME op class: a DBL step
 * (p2 + 4 squares) or an ADD step (p3 + 4 muls; ADD-A and ADD-B differ only
 * in where the table operand comes from).  With P >= 128 a full class
 * always exists (nA < 64 => nD > 64); at P = 112 nearly always.  Same field
 * ops as the reference, in the same order per signature: identical limbs.
 *
 *   k_ai    one lane per signature: k_dsm's activity check (-2 on an
 *           undecodable point) and Ai table of odd multiples of -A, plus
 *           the op-stream start init[i] = { -, heads, p|ja<<16|jb<<24, op }
 *           (heads: the top remaining h / s digit events, 0xffff = none).
 *   k_dsmp  one wave per workgroup, gridDim.x waves; waves claim
 *           signatures for their free pool slots from a shared counter.  A
 *           finished signature parks its final p1p1 in its own Ai slab.
 *   k_fin   one lane per signature: p1p1 -> p2 and the limb compare of
 *           fd_ed25519_user.c:417-425; work statistics.
 */
#ifndef FD_POOL_P
#define FD_POOL_P 112
#endif
enum { OP_D = 0, OP_AA = 1, OP_AB = 2, OP_EMPTY = 3, OP_NONE = 4 };

/* the base-point table in the Ai slab's row layout: entry e = rows
   [Z = 1 | Y-X | Y+X | 2dT] x 12 limbs (10 used), so ADD-A and ADD-B load
   their operand with the same code from different bases */
__device__ i32 g_bi12[8][48];
#ifdef FD_AMD_DIAG
__device__ u32 g_pool_dbg[5];   /* steps, live lanes, ADD steps, refill-only steps, ADD-only steps (summed over waves) */
__device__ u64 g_pool_dbg_t[8192][4];   /* per wave: wall_clock64 at start, at exhaustion of the counter, at exit; steps after exhaustion | lanes << 32 */
#endif

#ifndef FD_AI_WAVES
#define FD_AI_WAVES 2
#endif
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(FD_AI_WAVES)))
k_ai( u32 n, i8 * __restrict__ err, u8 * __restrict__ ws, ws_layout_t L ) {
  if( blockIdx.x == 0 ) {
    for( int k=threadIdx.x; k<8*48; k+=64 ) {
      int e = k / 48, c = (k % 48) / 12, l = k % 12;
      i32 v = 0;
      if( l < 10 ) {
        if( c == 0 ) v = (l == 0);
        else if( c == 1 ) v = BI_TABLE[e][1][l];
        else if( c == 2 ) v = BI_TABLE[e][0][l];
        else v = BI_TABLE[e][2][l];
      }
      g_bi12[e][k % 48] = v;
    }
  }
  u32 i = blockIdx.x * 64u + threadIdx.x;
  if( i == 0u ) { ((u32 *)(ws + L.ctr))[0] = 0u; ((u32 *)(ws + L.ctr))[1] = 0u; }   /* work counter, guard flag */
  bool act = (i < n) && (err[i] == 1);
  if( act && (ws[L.ds + 2u*i] | ws[L.ds + 2u*i + 1u]) ) { err[i] = (i8)-2; act = false; }
  size_t N = L.N;
  u32 ii = (i < n) ? i : 0u;
  /* the wave's 64 tables are written one entry at a time through LDS: lane
     l stages its 192-B entry, then the wave stores the 64 entries as 12
     contiguous 1-KB rows (whole 64-B lines; a lane writing its own table
     touches 64 lines per store and took ~0.36 of k_ai's 0.78 ms).  Lanes past
     n or inactive write don't-care tables into their own slabs (< N, never
     read). */
  __shared__ int4 s_ai[64 * 13];                   /* 13: a lane's entry starts 52 dwords after the last one's */
  int4 * const s_me = s_ai + threadIdx.x * 13u;
  int4 * const Ab = (int4 *)((i32 *)(ws + L.Ai) + (size_t)blockIdx.x * 64u * 384u);
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
#   define AI_ROW( r, f ) do {                                                      \
      s_me[3*(r)  ] = make_int4( f.v[0], f.v[1], f.v[2], f.v[3] );                  \
      s_me[3*(r)+1] = make_int4( f.v[4], f.v[5], f.v[6], f.v[7] );                  \
      s_me[3*(r)+2] = make_int4( f.v[8], f.v[9], 0, 0 );                            \
    } while(0)
#   define AI_STORE( e ) do {                                                       \
      AI_ROW( 0, cZ ); AI_ROW( 1, cYmX ); AI_ROW( 2, cYpX ); AI_ROW( 3, cT2d );     \
      __syncthreads();                                                              \
      _Pragma("unroll") for( u32 q=0; q<12u; q++ ) {                                \
        u32 const x = q*64u + threadIdx.x, sg = x / 12u, c = x - 12u*sg;            \
        Ab[(size_t)sg*96u + (e)*12u + c] = s_ai[sg*13u + c];                        \
      }                                                                             \
      __syncthreads();                                                              \
    } while(0)
    AI_STORE( 0u );
    p1p1 t = ge_dbl( A.X, A.Y, A.Z );
    p3 A2 = ge_p1p1_to_p3( t );
    for( u32 e=0; e<7u; e++ ) {
      p1p1 s2 = ge_add<false>( A2, cZ, cYmX, cYpX, cT2d, false );
      p3 u = ge_p1p1_to_p3( s2 );
      ge_to_cached( cZ, cYmX, cYpX, cT2d, u );
      AI_STORE( e+1u );
    }
#   undef AI_STORE
#   undef AI_ROW
  }
  if( i < n ) {
    uint4 in = make_uint4( 0u, 0xffffffffu, 0u, (u32)OP_EMPTY );
    int p = act ? ((int const *)(ws + L.top))[i] : -1;
    if( p >= 0 ) {
      u32 ne = ((u32 const *)(ws + L.evn))[i];
      u32 na = ne & 0xffu, nb = (ne >> 8) & 0xffu;
      u16 const * ev = (u16 const *)(ws + L.dig) + (size_t)i*128u;
      u32 hA = na ? (u32)ev[na - 1u] : 0xffffu, hB = nb ? (u32)ev[64u + nb - 1u] : 0xffffu;
      in = make_uint4( 0u, hA | (hB << 16), ((u32)p & 0xffffu) | (na << 16) | (nb << 24), (u32)OP_D );
    }
    ((uint4 *)(ws + L.init))[i] = in;
  }
}

__device__ __forceinline__ void
pool_load_t( p1p1 & t, int4 const * s ) {
  _Pragma("unroll") for( int r=0; r<10; r++ ) {
    int4 x = s[r];
    i32 v[4] = { x.x, x.y, x.z, x.w };
    _Pragma("unroll") for( int c=0; c<4; c++ ) {
      int k = 4*r + c;                     /* limb k of [X | Y | Z | T] */
      if( k < 10 ) t.X.v[k] = v[c]; else if( k < 20 ) t.Y.v[k-10] = v[c];
      else if( k < 30 ) t.Z.v[k-20] = v[c]; else t.T.v[k-30] = v[c];
    }
  }
}

__device__ __forceinline__ void
pool_store_t( int4 * s, p1p1 const & t ) {
  _Pragma("unroll") for( int r=0; r<10; r++ ) {
    i32 v[4];
    _Pragma("unroll") for( int c=0; c<4; c++ ) {
      int k = 4*r + c;
      v[c] = (k < 10) ? t.X.v[k] : (k < 20) ? t.Y.v[k-10] : (k < 30) ? t.Z.v[k-20] : t.T.v[k-30];
    }
    s[r] = make_int4( v[0], v[1], v[2], v[3] );
  }
}

template<typename PTR>
__device__ __forceinline__ void
pool_load_ts( p1p1 & t, PTR s, u32 stride ) {
  _Pragma("unroll") for( int r=0; r<10; r++ ) {
    int4 x = s[(u32)r * stride];
    i32 v[4] = { x.x, x.y, x.z, x.w };
    _Pragma("unroll") for( int c=0; c<4; c++ ) {
      int k = 4*r + c;
      if( k < 10 ) t.X.v[k] = v[c]; else if( k < 20 ) t.Y.v[k-10] = v[c];
      else if( k < 30 ) t.Z.v[k-20] = v[c]; else t.T.v[k-30] = v[c];
    }
  }
}

template<typename PTR>
__device__ __forceinline__ void
pool_store_ts( PTR s, u32 stride, p1p1 const & t ) {
  _Pragma("unroll") for( int r=0; r<10; r++ ) {
    i32 v[4];
    _Pragma("unroll") for( int c=0; c<4; c++ ) {
      int k = 4*r + c;
      v[c] = (k < 10) ? t.X.v[k] : (k < 20) ? t.Y.v[k-10] : (k < 30) ? t.Z.v[k-20] : t.T.v[k-30];
    }
    s[(u32)r * stride] = make_int4( v[0], v[1], v[2], v[3] );
  }
}

/* a pure DBL step is chosen while its lane count is at least this percentage
   of a mixed step's.  100: only a full DBL step (64 lanes) beats a mixed one.
   The steps' cost ratio (~0.72) was the round-2 setting (78); a model of the
   pool's op streams and an interleaved A/B both favour 100: ADD slots wait
   less, so fewer signatures sit in the pool with nothing but an ADD to do
   (DSM stage -1 to -2 %, profiles/r03_pool_tune_ab.txt) */
#ifndef FD_POOL_DBL_PCT
#define FD_POOL_DBL_PCT 100u
#endif
/* k_dsmp's drain: issue priority by the signatures left in the pool */
#ifndef FD_POOL_DRAIN_PRIO
#define FD_POOL_DRAIN_PRIO 1
#endif
/* free slots that trigger a refill (one counter atomic + init loads) */
#ifndef FD_POOL_REFILL
#define FD_POOL_REFILL 8u
#endif

/* The mixed step's op on one lane's p1p1 state: k_dsm's uniform 8-mul step
   (p1p1 -> p3, then the ADD's or the DBL's four products as general muls,
   operands selected per lane).  HAS_DBL false is the same step for a
   selection that holds no DBL slot: the DBL lane mask is the constant 0, so
   every select keeps its ADD arm and folds away.  There a dead lane
   (live false) reads g_bi12[0], as a DBL lane does in the general step; the
   caller stores nothing for it. */
template<bool HAS_DBL>
__device__ __forceinline__ i32 pool_vsel( u64 mD, i32 d, i32 a ) { return HAS_DBL ? vsel( mD, d, a ) : a; }

template<bool HAS_DBL>
__device__ __forceinline__ void
pool_mixed_body( p1p1 & t, u32 op, u32 hA, u32 hB, u32 si, bool live, i32 const * Ai ) {
  bool isadd = HAS_DBL ? (op == OP_AA || op == OP_AB) : live;
  int dg = (op == OP_AA) ? (int)(i8)(hA >> 8) : (int)(i8)(hB >> 8);
  bool neg = isadd && dg < 0;
  int e = isadd ? ((dg < 0 ? -dg : dg) >> 1) & 7 : 0;
  i32 const * qb = (op == OP_AA) ? Ai + (size_t)si*384u + e*48 : &g_bi12[e][0];
  int const rowM = neg ? 2 : 1, rowP = neg ? 1 : 2;
  fe q[4];
# define Q_ROW( R_, C_ ) do {                                                     \
    int4 const * src_ = (int4 const *)(qb + (C_)*12);                            \
    int4 x0 = src_[0], x1 = src_[1], x2 = src_[2];                               \
    q[R_].v[0] = x0.x; q[R_].v[1] = x0.y; q[R_].v[2] = x0.z; q[R_].v[3] = x0.w;  \
    q[R_].v[4] = x1.x; q[R_].v[5] = x1.y; q[R_].v[6] = x1.z; q[R_].v[7] = x1.w;  \
    q[R_].v[8] = x2.x; q[R_].v[9] = x2.y;                                        \
  } while(0)
  Q_ROW( 0, 0 ); Q_ROW( 1, rowM ); Q_ROW( 2, rowP ); Q_ROW( 3, 3 );
# undef Q_ROW
  p3 u = ge_p1p1_to_p3_fold( t );
  /* the table operand is first touched here, after p1p1 -> p3 (its x19
     pre-multiples would otherwise be scheduled first and wait for it) */
  _Pragma("unroll") for( int r=0; r<4; r++ )
    asm volatile( "" : "+v"(q[r].v[0]), "+v"(q[r].v[1]), "+v"(q[r].v[2]), "+v"(q[r].v[3]), "+v"(q[r].v[4]),
                       "+v"(q[r].v[5]), "+v"(q[r].v[6]), "+v"(q[r].v[7]), "+v"(q[r].v[8]), "+v"(q[r].v[9])
                     : "v"(u.X.v[9]), "v"(u.T.v[9]) );
  /* k_dsm's op body and mix (see k_dsm) */
  u64 const mD = HAS_DBL ? __builtin_amdgcn_ballot_w64( !isadd ) : 0UL, mN = __builtin_amdgcn_ballot_w64( neg );
  fe m0, m1, m2, m3;
  {
    fe a0, b0, a1, b1, a2, b2, a3, b3;
    _Pragma("unroll") for( int k=0; k<10; k++ ) {
      i32 xy = u.X.v[k] + u.Y.v[k];
      a0.v[k] = xy;                                                        b0.v[k] = pool_vsel<HAS_DBL>( mD, xy, q[2].v[k] );
      a1.v[k] = pool_vsel<HAS_DBL>( mD, u.Y.v[k], u.Y.v[k] - u.X.v[k] );   b1.v[k] = pool_vsel<HAS_DBL>( mD, u.Y.v[k], q[1].v[k] );
      a2.v[k] = u.Z.v[k];                                                  b2.v[k] = pool_vsel<HAS_DBL>( mD, u.Z.v[k] + u.Z.v[k], q[0].v[k] );
      a3.v[k] = pool_vsel<HAS_DBL>( mD, u.X.v[k], u.T.v[k] );              b3.v[k] = pool_vsel<HAS_DBL>( mD, u.X.v[k], q[3].v[k] );
    }
    fe_mul_fold2w<true, true>( m0, a0, b0, m1, a1, b1 );
    fe_mul_fold2w<false, true>( m2, a2, b2, m3, a3, b3 );
  }
  {
    u64 mS = mD | mN;
    i32 Dv = pool_vsel<HAS_DBL>( mD, -1, 0 ), Sv = vsel( mS, -1, 0 ), Sn = vsel( mS, 1, 0 );
    i32 cXe = Dv & (1<<25), cXo = Dv & (1<<24);
    i32 cZe = pool_vsel<HAS_DBL>( mD, 0, vsel( mN, (1<<25), -(1<<25) ) ), cZo = pool_vsel<HAS_DBL>( mD, 0, vsel( mN, (1<<24), -(1<<24) ) );
    i32 const nb2e = (i32)fd_opaque( -(2L<<25) ), nb2o = (i32)fd_opaque( -(2L<<24) );   /* SGPR */
    i32 const sT = pool_vsel<HAS_DBL>( mD, 0, 2 );
    _Pragma("unroll") for( int k=0; k<10; k++ ) {
      i32 cX = (k & 1) ? cXo : cXe, cZ = (k & 1) ? cZo : cZe;
      i32 A0 = m0.v[k], A1 = m1.v[k], A2 = m2.v[k], A3 = m3.v[k];
      i32 sA3 = fd_xad( A3, Sv, Sn );
      i32 z2 = A2 + A2;
      i32 Z = fd_add3( pool_vsel<HAS_DBL>( mD, A1, z2 ), sA3, cZ );
      t.X.v[k] = HAS_DBL ? fd_add3( A0 - A1, sA3 & Dv, cX ) : A0 - A1;   /* ADD: X = m0 - m1 */
      t.Y.v[k] = fd_add3s( A1, pool_vsel<HAS_DBL>( mD, A3, A0 ), (k & 1) ? nb2o : nb2e );
      t.Z.v[k] = Z;
      t.T.v[k] = (i32)((u32)A2 << (u32)sT) - Z;
    }
  }
}


__device__ __forceinline__ u32 lane_rank( u64 m ) {   /* set bits of m below this lane */
  return __builtin_amdgcn_mbcnt_hi( (u32)(m >> 32), __builtin_amdgcn_mbcnt_lo( (u32)m, 0u ) );
}

/* The pool's op classes live in four wave-uniform 64-bit masks (slot s is
   bit s & 63 of word s >> 6): mD = DBL next, mA = ADD-A / ADD-B next,
   neither = free.  A step takes the first (up to) 64 slots of one class in
   slot order; lane l learns the l-th of them from a rank list in LDS, loads
   its slot's state from LDS, runs the op and writes the state back; the slots'
   new classes return to the masks through each slot's owner lane (s & 63),
   which pulls the processing lane's verdict with ds_bpermute. */
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2)))
k_dsmp( u32 n, u8 * __restrict__ ws, ws_layout_t L, u64 iter_cap ) {
  constexpr u32 P = FD_POOL_P;
  static_assert( P >= 64 && P <= 128, "pool: each lane owns slots l and l + 64" );
  __shared__ int4  s_t[10][P];   /* p1p1 state [X | Y | Z | T], 16-B column r of slot s at [r][s]:
                                    a lane's b128 starts at bank 4 (s mod 16), not 8 (s mod 8) */
  __shared__ uint4 s_m[P];       /* { sig, heads, p | ja<<16 | jb<<24, op } */
  __shared__ u32   s_list[64];   /* slot of each rank in the step's selection */
  u32 const l = threadIdx.x, w = blockIdx.x;
  uint4 const * init = (uint4 const *)(ws + L.init);
  u16 const * dig = (u16 const *)(ws + L.dig);
  i32 * Ai = (i32 *)(ws + L.Ai);
  u64 const valid1 = (P >= 128u) ? ~0UL : ((1UL << (P - 64u)) - 1UL);   /* slots 64.. that exist */

  u64 mD0 = 0, mD1 = 0, mA0 = 0, mA1 = 0;
#ifdef FD_AMD_DIAG
  u64 dbg_t0 = wall_clock64(), dbg_te = 0; bool dbg_after = false; u64 dbg_sa = 0, dbg_la = 0;
#endif
  u32 * ctr = (u32 *)(ws + L.ctr);   /* next unclaimed signature, shared by all waves */
  bool more = true;                  /* wave-uniform: the counter has not passed n */
  /* hang guard: every step advances at least one op of at most 448 per
     signature, and a wave can claim at most all n signatures.  A wave that
     reaches it raises the launch's guard flag: k_fin then marks every
     verdict FD_AMD_VERDICT_DEVICE and the host call fails with
     FD_ED25519_AMD_ERR_DEVICE (iter_cap: a debug cap, ~0 normally). */
  u64 iter_max = ((u64)n + 2u*P) * 448u;
  if( iter_cap < iter_max ) iter_max = iter_cap;
  bool guard = true;
#ifdef FD_AMD_DIAG
  u32 dbg_steps = 0, dbg_lanes = 0, dbg_add = 0, dbg_idle = 0, dbg_addonly = 0;
#endif
  for( u64 iter = 0; iter < iter_max; iter++ ) {
    u32 nD = (u32)(__builtin_popcountll( mD0 ) + __builtin_popcountll( mD1 ));
    u32 nA = (u32)(__builtin_popcountll( mA0 ) + __builtin_popcountll( mA1 ));
    u64 f0 = ~(mD0 | mA0), f1 = ~(mD1 | mA1) & valid1;   /* free slots */
    u32 nfree = (u32)(__builtin_popcountll( f0 ) + __builtin_popcountll( f1 ));
    /* refill in batches (one global round trip per 16 finished signatures),
       or whenever no class fills a wave */
    if( more && nfree && (nfree >= FD_POOL_REFILL || (nD < 64u && nA < 64u)) ) {
#ifdef FD_AMD_DIAG
      dbg_idle++;
#endif
      /* claim nfree signatures (one vector atomic; faster waves claim more,
         so the waves of a launch finish together) */
      u32 base = 0u;
      if( l == 0u ) base = atomicAdd( ctr, nfree );
      base = (u32)__builtin_amdgcn_readfirstlane( (int)base );
      if( base + nfree >= n || base + nfree < base ) {
        more = false;
#ifdef FD_AMD_DIAG
        dbg_te = wall_clock64(); dbg_after = true;
#endif
      }
      u32 pf0 = (u32)__builtin_popcountll( f0 );
      u64 s0 = (u64)base + lane_rank( f0 ), s1 = (u64)base + pf0 + lane_rank( f1 );
      bool r0 = ((f0 >> l) & 1u) && s0 < n, r1 = ((f1 >> l) & 1u) && s1 < n;
      uint4 in0 = init[r0 ? s0 : 0u], in1 = init[r1 ? s1 : 0u];
      r0 = r0 && in0.w == OP_D; r1 = r1 && in1.w == OP_D;   /* inactive signatures leave the slot free */
      p1p1 id;   /* new signatures enter with the identity (p1p1 whose p2 is (0,1,1)) */
      id.X = fe_zero(); id.Y = fe_one(); id.Z = fe_one(); id.T = fe_one();
      if( r0 ) { s_m[l] = make_uint4( (u32)s0, in0.y, in0.z, (u32)OP_D ); pool_store_ts( &s_t[0][l], P, id ); }
      if( r1 ) { s_m[l + 64u] = make_uint4( (u32)s1, in1.y, in1.z, (u32)OP_D ); pool_store_ts( &s_t[0][l + 64u], P, id ); }
      mD0 |= __builtin_amdgcn_ballot_w64( r0 );
      mD1 |= __builtin_amdgcn_ballot_w64( r1 );
      nD = (u32)(__builtin_popcountll( mD0 ) + __builtin_popcountll( mD1 ));
    }
    if( !(nD + nA) ) {
      if( !more ) { guard = false; break; }   /* pool empty, nothing left to take */
      continue;
    }
#if FD_POOL_DRAIN_PRIO
    /* drain: the wave with more signatures left issues first on its SIMD
       (at equal priority the arbiter prefers the older wave, whatever its
       pool holds), so the two waves of a SIMD empty their pools together */
    if( !more ) {
      u32 const left = nD + nA;
      if( left > 84u )      __builtin_amdgcn_s_setprio( 3 );
      else if( left > 56u ) __builtin_amdgcn_s_setprio( 2 );
      else if( left > 28u ) __builtin_amdgcn_s_setprio( 1 );
      else                  __builtin_amdgcn_s_setprio( 0 );
    }
#endif

    u32 kD = nD < 64u ? nD : 64u, kM = (nD + nA) < 64u ? (nD + nA) : 64u;
    bool mixed;
    u32 nsel, rk0, rk1;
    u64 S0, S1;
    if( !more ) {
      /* drain (nothing left to claim): the pool's last signatures set the
         launch's end.  The class is chosen as in the main phase; within it
         the (up to) 64 slots with the most ops left, p + ja + jb (remaining
         doublings and adds), go first -- in a mixed step every ADD slot
         ranks above every DBL slot.  A threshold search on those counts (10
         ballots) finds the 64th largest; ties go in slot order.  (Slot
         order alone left the youngest signatures waiting: 393 / 620 steps
         after the counter ran out, median / max, vs 382 / 479.) */
      mixed = 100u * kD < FD_POOL_DBL_PCT * kM;
      u64 const L0 = mixed ? (mA0 | mD0) : mD0, L1 = mixed ? (mA1 | mD1) : mD1;
      u32 const K = mixed ? kM : kD;
      u32 const z0 = s_m[l].z, z1 = s_m[l + 64u < P ? l + 64u : l].z;
      u32 const r0 = (z0 & 0xffffu) + ((z0 >> 16) & 0xffu) + (z0 >> 24) + (u32)vsel( mixed ? mA0 : 0UL, 512, 0 );
      u32 const r1 = (z1 & 0xffffu) + ((z1 >> 16) & 0xffu) + (z1 >> 24) + (u32)vsel( mixed ? mA1 : 0UL, 512, 0 );
      u32 T = 0u;
      _Pragma("unroll") for( int b=9; b>=0; b-- ) {   /* keys are below 1024 */
        u32 const Tb = T | (1u << b);
        u32 const c = (u32)(__builtin_popcountll( L0 & __builtin_amdgcn_ballot_w64( r0 >= Tb ) ) +
                            __builtin_popcountll( L1 & __builtin_amdgcn_ballot_w64( r1 >= Tb ) ));
        T = c >= K ? Tb : T;
      }
      u64 const G0 = L0 & __builtin_amdgcn_ballot_w64( r0 > T ), G1 = L1 & __builtin_amdgcn_ballot_w64( r1 > T );
      u64 const E0 = L0 & ~G0 & __builtin_amdgcn_ballot_w64( r0 >= T ), E1 = L1 & ~G1 & __builtin_amdgcn_ballot_w64( r1 >= T );
      u32 const need = K - (u32)(__builtin_popcountll( G0 ) + __builtin_popcountll( G1 ));
      u32 const e0 = (u32)__builtin_popcountll( E0 );
      S0 = G0 | (E0 & __builtin_amdgcn_ballot_w64( lane_rank( E0 ) < need ));
      S1 = G1 | (E1 & __builtin_amdgcn_ballot_w64( e0 + lane_rank( E1 ) < need ));
      rk0 = lane_rank( S0 ); rk1 = (u32)__builtin_popcountll( S0 ) + lane_rank( S1 );
      nsel = K;
    } else {
      /* the step: a pure DBL step (p2 + 4 squares) on up to 64 DBL slots,
         or a MIXED step (k_dsm's uniform 8-mul step) that takes every ADD
         slot first and fills the rest with DBL slots.  An ADD op costs the
         same in either, so ADDs always go through mixed steps; a DBL step
         runs only when it fills the wave (FD_POOL_DBL_PCT 100). */
      mixed = 100u * kD < FD_POOL_DBL_PCT * kM;
      nsel = mixed ? kM : kD;
      /* owner view: the rank of my slots in the selection order [ADD slots
         0..63, ADD slots 64.., DBL slots 0..63, DBL slots 64..] (ADDs only
         in a mixed step) is their processing lane.  Class bits are the
         wave-uniform masks used as lane masks (inverse ballot, v_cndmask):
         no per-lane shifts of the masks. */
      u64 const sA0 = mixed ? mA0 : 0UL, sA1 = mixed ? mA1 : 0UL;
      u32 const aoff = mixed ? nA : 0u;                         /* DBL ranks start after the ADDs */
      u32 const pa0 = (u32)__builtin_popcountll( sA0 ), pd0 = (u32)__builtin_popcountll( mD0 );
      rk0 = (u32)vsel( sA0, (i32)lane_rank( sA0 ), (i32)(aoff + lane_rank( mD0 )) );
      rk1 = (u32)vsel( sA1, (i32)(pa0 + lane_rank( sA1 )), (i32)(aoff + pd0 + lane_rank( mD1 )) );
      S0 = (sA0 | mD0) & __builtin_amdgcn_ballot_w64( rk0 < 64u );
      S1 = (sA1 | mD1) & __builtin_amdgcn_ballot_w64( rk1 < 64u );
    }
    bool in0 = __builtin_amdgcn_inverse_ballot_w64( S0 ), in1 = __builtin_amdgcn_inverse_ballot_w64( S1 );
    bool const hasD = ((S0 & mD0) | (S1 & mD1)) != 0UL;   /* a mixed step without a DBL slot runs the ADD-only body */
    mA0 &= ~S0; mA1 &= ~S1; mD0 &= ~S0; mD1 &= ~S1;
#ifdef FD_AMD_DIAG
    dbg_steps++; dbg_lanes += nsel; dbg_add += mixed; dbg_addonly += mixed && !hasD;
    if( dbg_after ) { dbg_sa++; dbg_la += nsel; }
#endif
    bool live = l < nsel;
    /* slot of rank l: each selected slot's owner writes it at its rank (the
       wave's LDS accesses complete in order: no barrier for a one-wave group) */
    if( in0 ) s_list[rk0] = l;
    if( in1 ) s_list[rk1] = l + 64u;
    __builtin_amdgcn_wave_barrier();
    u32 s = live ? s_list[l] : 0u;
    uint4 m = s_m[s];
    u32 op = live ? m.w : (u32)OP_D;    /* dead lanes: harmless reads, nothing stored */
    u32 si = live ? m.x : 0u;
    u32 hA = m.y & 0xffffu, hB = m.y >> 16;
    int p = (int)(short)(m.z & 0xffffu);
    u32 ja = (m.z >> 16) & 0xffu, jb = m.z >> 24;
    p1p1 t;
    pool_load_ts( t, &s_t[0][s], P );

    /* the op, then the op stream's advance: pop the consumed event (only an
       ADD consumes one, so only a mixed step runs the pop path; `mixed` is
       wave-uniform), then the next op (branch-free: every select is a lane
       mask) */
    bool toAA, toAB;
    if( mixed ) {
      /* the consumed event's successor (popped after the op): its dword */
      u32 pidx = (op == OP_AA && ja >= 2u) ? ja - 2u : (op == OP_AB && jb >= 2u) ? 64u + jb - 2u : 0u;
      bool pop = (op == OP_AA && ja >= 2u) || (op == OP_AB && jb >= 2u);
      /* lanes that pop nothing read one shared, cache-resident word instead of
         their own event row (a load under a divergent branch would wait at
         the join) */
      u32 const * nha = pop ? (u32 const *)(dig + (size_t)si*128u) + (pidx >> 1) : (u32 const *)&g_bi12[0][0];
      u32 nh = *nha;
      if( hasD ) pool_mixed_body<true>( t, op, hA, hB, si, live, Ai );
      else       pool_mixed_body<false>( t, op, hA, hB, si, live, Ai );
      bool const isAA = op == OP_AA, isAB = op == OP_AB, isDb = op == OP_D;
      u32 ev = __builtin_amdgcn_ubfe( nh, (pidx & 1u) << 4, 16u );
      ja -= (u32)isAA; jb -= (u32)isAB;
      hA = isAA ? (ja ? ev : 0xffffu) : hA;
      hB = isAB ? (jb ? ev : 0xffffu) : hB;
      toAA = isDb && hA != 0xffffu && (hA & 0xffu) == (u32)p;
      toAB = !toAA && (isDb || isAA) && hB != 0xffffu && (hB & 0xffu) == (u32)p;
    } else {
      /* p1p1 -> p2 (the first three products of p1p1 -> p3), then the
         doubling (avx/fd_ed25519_ge.c:493-498) with squares */
      fe uZ, uY, uX;
      fe_mul_fold2w( uZ, t.Z, t.T, uY, t.Z, t.Y );
      uX = fe_mul_fold1( t.X, t.T );
      fe xy = fe_add( uX, uY );
      fe a, b, c, d;
      fe_sq_fold2w<false, false>( a, xy, b, uY );
      fe_sq_fold2w<false, true>( c, uX, d, uZ );
      _Pragma("unroll") for( int k=0; k<10; k++ ) {
        i32 z = b.v[k] - c.v[k];
        t.X.v[k] = a.v[k] - b.v[k] - c.v[k];
        t.Y.v[k] = b.v[k] + c.v[k];
        t.Z.v[k] = z;
        t.T.v[k] = d.v[k] - z;
      }
      /* every selected slot's op is a doubling: heads and counts stay */
      toAA = hA != 0xffffu && (hA & 0xffu) == (u32)p;
      toAB = !toAA && hB != 0xffffu && (hB & 0xffu) == (u32)p;
    }
    p -= (int)!(toAA || toAB);
    u32 nop = !live ? (u32)OP_EMPTY : toAA ? (u32)OP_AA : toAB ? (u32)OP_AB : (p < 0) ? (u32)OP_EMPTY : (u32)OP_D;
    if( live ) {
      if( nop == OP_EMPTY ) {
        pool_store_t( (int4 *)(Ai + (size_t)si*384u), t );   /* park the final p1p1 for k_fin */
      } else {
        pool_store_ts( &s_t[0][s], P, t );
        s_m[s] = make_uint4( si, hA | (hB << 16), ((u32)p & 0xffffu) | (ja << 16) | (jb << 24), nop );
      }
    }
    /* the slots' new classes, at their owner lanes */
    u32 v0 = (u32)__builtin_amdgcn_ds_bpermute( (int)(rk0 << 2), (int)nop );
    u32 v1 = (u32)__builtin_amdgcn_ds_bpermute( (int)((rk1 & 63u) << 2), (int)nop );
    u64 const d0 = __builtin_amdgcn_ballot_w64( v0 == OP_D ), d1 = __builtin_amdgcn_ballot_w64( v1 == OP_D );
    u64 const x0 = __builtin_amdgcn_ballot_w64( v0 < OP_EMPTY ), x1 = __builtin_amdgcn_ballot_w64( v1 < OP_EMPTY );
    mD0 |= S0 & d0; mA0 |= S0 & x0 & ~d0;                       /* OP_AA / OP_AB: below OP_EMPTY, not OP_D */
    mD1 |= S1 & d1; mA1 |= S1 & x1 & ~d1;
  }
  if( guard && l == 0u ) atomicOr( (u32 *)(ws + L.ctr) + 1, 1u );
#ifdef FD_AMD_DIAG
  if( l == 0u ) { atomicAdd( &g_pool_dbg[0], dbg_steps ); atomicAdd( &g_pool_dbg[1], dbg_lanes ); atomicAdd( &g_pool_dbg[2], dbg_add ); atomicAdd( &g_pool_dbg[3], dbg_idle ); atomicAdd( &g_pool_dbg[4], dbg_addonly ); }
  if( l == 0u && w < 8192u ) { g_pool_dbg_t[w][0] = dbg_t0; g_pool_dbg_t[w][1] = dbg_te; g_pool_dbg_t[w][2] = wall_clock64(); g_pool_dbg_t[w][3] = dbg_sa | (dbg_la << 32); }
#else
  (void)w;
#endif
}

#ifdef FD_AMD_DIAG
extern "C" int
fd_amd_pool_debug( unsigned * out, int reset ) {
  if( hipMemcpyFromSymbol( out, HIP_SYMBOL( g_pool_dbg ), sizeof(unsigned)*5 ) != hipSuccess ) return -1;
  if( reset ) { unsigned z[5] = { 0, 0, 0, 0, 0 }; if( hipMemcpyToSymbol( HIP_SYMBOL( g_pool_dbg ), z, sizeof(z) ) != hipSuccess ) return -1; }
  return 0;
}
extern "C" int
fd_amd_pool_debug_times( unsigned long * out /* [8192][4] */ ) {
  return hipMemcpyFromSymbol( out, HIP_SYMBOL( g_pool_dbg_t ), sizeof(unsigned long)*8192*4 ) == hipSuccess ? 0 : -1;
}
#endif

__global__ void __launch_bounds__(64)
k_fin( u32 n, i8 * __restrict__ err, u8 * __restrict__ ws, ws_layout_t L, int want_stats ) {
  u32 i = blockIdx.x * 64u + threadIdx.x;
  if( i >= n ) return;
  size_t N = L.N;
  if( ((u32 const *)(ws + L.ctr))[1] ) { err[i] = (i8)FD_AMD_VERDICT_DEVICE; return; }   /* k_dsmp's guard tripped */
  bool act = err[i] == 1;
  int top = ((int const *)(ws + L.top))[i];
  if( act ) {
    p1p1 t;
    if( top < 0 ) { t.X = fe_zero(); t.Y = fe_one(); t.Z = fe_one(); t.T = fe_one(); }
    else pool_load_t( t, (int4 const *)((i32 const *)(ws + L.Ai) + (size_t)i*384u) );
    fe uZ, uY, uX;
    fe_mul_fold2w( uZ, t.Z, t.T, uY, t.Z, t.Y );
    uX = fe_mul_fold1( t.X, t.T );
    i32 const * Rw = (i32 const *)(ws + L.R);
    fe RX, RY;
    _Pragma("unroll") for( int k=0; k<10; k++ ) { RX.v[k] = Rw[(size_t)k*N + i]; RY.v[k] = Rw[(size_t)(10+k)*N + i]; }
    fe xZ, yZ;
    fe_mul_fold2w( xZ, uZ, RX, yZ, uZ, RY );
    bool eq = true;
    _Pragma("unroll") for( int k=0; k<8; k++ ) eq = eq && (xZ.v[k] == uX.v[k]) && (yZ.v[k] == uY.v[k]);
    err[i] = (i8)(eq ? 0 : -3);
  }
  if( want_stats ) {
    u32 ne = ((u32 const *)(ws + L.evn))[i];
    u32 * st = (u32 *)(ws + L.st);
    st[i] = act ? (u32)(top + 1) : 0u; st[N + i] = act ? (ne & 0xffu) : 0u; st[2*N + i] = act ? ((ne >> 8) & 0xffu) : 0u;
  }
}

/* The R' = (X, Y, Z) of a signature after k_dsmp, for a kernel that runs
   after k_fin (k_strict): the final p1p1 that pool_store_t parked in the
   signature's Ai slab, turned into X, Y, Z with k_fin's three products; a
   signature with no digit at all (top < 0: h = s = 0) never entered the
   pool and parked nothing, its R' is the identity, as in k_fin.  Only for
   signatures that were pending when k_ai ran, and never after the step
   guard tripped (the slabs are then unfinished). */
__device__ __forceinline__ void
pool_load_parked( fe & X, fe & Y, fe & Z, i32 const * __restrict__ Ail, int top ) {
  p1p1 t;
  if( top < 0 ) { t.X = fe_zero(); t.Y = fe_one(); t.Z = fe_one(); t.T = fe_one(); }
  else pool_load_t( t, (int4 const *)Ail );
  fe_mul_fold2w( Z, t.Z, t.T, Y, t.Z, t.Y );
  X = fe_mul_fold1( t.X, t.T );
}

#endif /* FD_ED25519_POOL_H */
