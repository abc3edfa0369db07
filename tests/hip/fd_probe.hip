/* tests/hip/fd_probe.hip
 *
 * TEST INFRASTRUCTURE ONLY -- probe kernels around the device field / group
 * functions of the verify engine, so that tests/test_field_probe_gpu.py can
 * compare every variant limb for limb with the Python model of the
 * reference's arithmetic (tests/_fe_ref.py) on directed inputs, and around
 * the device functions of the GPU signer (the sign_* ops), which
 * tests/test_sign_probe_gpu.py compares with plain integer arithmetic and
 * the RFC 8032 model of tests/_sign_ref.py.
 *
 * Only the product's stage headers that hold the probed functions are
 * included, verbatim: the field ops (fd_ed25519_dev.h), the group ops,
 * quad and half helpers (fd_ed25519_dsm8.h, which brings in dsm4 and dsm)
 * and the signer's device functions (fd_ed25519_sign.h).
 * The front, the pool, the tile kernel, k_sign and the launch code are not
 * compiled here; nothing here is linked into the product library.  Every
 * probe is straight-line code (fixed trip counts only; the one exception is
 * fe_sq_iter's fixed squaring counts inside the signer's fe_invert) on
 * whole 64-lane waves: the case count is padded with all-zero cases so
 * every lane is active (the DPP forms read neighbour lanes).
 *
 * Layout: arrays are case-major, [case][stride] int32.  An op's shape is
 * { lanes per case, in0 / in1 / aux / out ints per case } (fd_probe_shape).
 *   1-lane ops : case k on lane k
 *   quad ops   : case k on lanes 4k..4k+3; per-lane data is [lane][10]
 *   8-lane ops : case k on lanes 8k..8k+7, half = (lane >> 2) & 1 with
 *                half_ctx built as dsm8_body builds it
 */

#include "../../firedancer_amd/csrc/fd_ed25519_dev.h"
#include "../../firedancer_amd/csrc/fd_ed25519_dsm8.h"
#include "../../firedancer_amd/csrc/fd_ed25519_sign.h"

enum {
  P_MUL = 0, P_MUL_FOLD1, P_MUL_ONE, P_SQN1, P_SQN2, P_SQ_FOLD,
  P_MUL_FOLD2W_00, P_MUL_FOLD2W_01, P_MUL_FOLD2W_10, P_MUL_FOLD2W_11,
  P_SQ_FOLD2W_00, P_SQ_FOLD2W_01, P_SQ_FOLD2W_10, P_SQ_FOLD2W_11,
  P_MUL_HALF5, P_POW22523, P_FROMBYTES, P_ISNONZERO, P_ISNEGATIVE, P_SC_REDUCE,
  P_GE_DBL, P_GE_P3, P_GE_P3_FOLD, P_GE_ADD, P_GE_MADD, P_GE_TO_CACHED,
  P_QUAD_P3, P_QUAD_BODY, P_QUAD_OWNC, P_QUAD8_OWNC5, P_QUAD_CACHED_ROW,
  P_SIGN_FE_INVERT, P_SIGN_FE_TOBYTES, P_SIGN_RECODE, P_SIGN_SCALARMULT_BASE, P_SIGN_SC_MULADD,
  P_OP_CNT
};

struct probe_shape_t { int lanes, s0, s1, sa, so; };

__host__ __device__ constexpr probe_shape_t
probe_shape( int op ) {
  switch( op ) {
  case P_MUL: case P_MUL_FOLD1:                      return { 1, 10, 10, 0, 10 };
  case P_MUL_ONE: case P_SQN1: case P_SQN2: case P_SQ_FOLD: case P_POW22523:
                                                     return { 1, 10, 0, 0, 10 };
  case P_MUL_FOLD2W_00: case P_MUL_FOLD2W_01: case P_MUL_FOLD2W_10: case P_MUL_FOLD2W_11:
                                                     return { 1, 20, 20, 0, 20 };   /* F1|F2, G1|G2 -> R1|R2 */
  case P_SQ_FOLD2W_00: case P_SQ_FOLD2W_01: case P_SQ_FOLD2W_10: case P_SQ_FOLD2W_11:
                                                     return { 1, 20, 0, 0, 20 };    /* F1|F2 -> R1|R2 */
  case P_MUL_HALF5:                                  return { 8, 10, 10, 0, 80 };   /* the joined element of each lane */
  case P_FROMBYTES:                                  return { 1, 8, 0, 0, 10 };
  case P_ISNONZERO: case P_ISNEGATIVE:               return { 1, 10, 0, 0, 1 };
  case P_SC_REDUCE:                                  return { 1, 16, 0, 0, 8 };
  case P_GE_DBL:                                     return { 1, 30, 0, 0, 40 };    /* X|Y|Z -> p1p1 X|Y|Z|T */
  case P_GE_P3: case P_GE_P3_FOLD:                   return { 1, 40, 0, 0, 40 };    /* p1p1 -> p3 X|Y|Z|T */
  case P_GE_ADD: case P_GE_MADD:                     return { 1, 40, 40, 1, 40 };   /* p3, [qZ|qYmX|qYpX|qT2d], neg -> p1p1 */
  case P_GE_TO_CACHED:                               return { 1, 40, 0, 0, 40 };    /* p3 -> [Z|YmX|YpX|T2d] */
  case P_QUAD_P3:                                    return { 4, 40, 0, 0, 160 };   /* p1p1 -> every lane's p3 */
  case P_QUAD_BODY:                                  return { 4, 40, 40, 2, 160 };  /* p3, qrow[lane], {isD, neg} -> every lane's p1p1 */
  case P_QUAD_OWNC:                                  return { 4, 40, 40, 2, 80 };   /* C[lane], qrow[lane], {isD, neg} -> pm[lane] | C'[lane] */
  case P_QUAD8_OWNC5:                                return { 8, 40, 40, 2, 160 };  /* the same on 8 lanes: pm[lane] (joined) | C'[lane] */
  case P_QUAD_CACHED_ROW:                            return { 4, 40, 0, 0, 40 };    /* p3 -> row[lane] */
  case P_SIGN_FE_INVERT:                             return { 1, 10, 0, 0, 10 };
  case P_SIGN_FE_TOBYTES:                            return { 1, 10, 0, 0, 8 };     /* limbs -> 8 LE words */
  case P_SIGN_RECODE:                                return { 1, 8, 0, 0, 16 };     /* scalar words -> 64 int8 digits, 4 per word */
  case P_SIGN_SCALARMULT_BASE:                       return { 1, 8, 0, 0, 8 };      /* scalar words -> encoded point */
  case P_SIGN_SC_MULADD:                             return { 1, 16, 8, 0, 8 };     /* k|a, r -> (r + k a) mod L */
  default:                                           return { 0, 0, 0, 0, 0 };
  }
}

static char const * const probe_names[P_OP_CNT] = {
  "fe_mul", "fe_mul_fold1", "fe_mul_one", "fe_sqn1", "fe_sqn2", "fe_sq_fold",
  "fe_mul_fold2w_00", "fe_mul_fold2w_01", "fe_mul_fold2w_10", "fe_mul_fold2w_11",
  "fe_sq_fold2w_00", "fe_sq_fold2w_01", "fe_sq_fold2w_10", "fe_sq_fold2w_11",
  "fe_mul_half5", "fe_pow22523", "fe_frombytes", "fe_isnonzero", "fe_isnegative", "sc_reduce",
  "ge_dbl", "ge_p1p1_to_p3", "ge_p1p1_to_p3_fold", "ge_add", "ge_madd", "ge_to_cached",
  "quad_p3", "quad_body", "quad_ownc", "quad8_ownc5", "quad_cached_row",
  "sign_fe_invert", "sign_fe_tobytes", "sign_recode", "sign_scalarmult_base", "sign_sc_muladd",
};

__device__ __forceinline__ fe   ldfe( i32 const * p ) { fe r; _Pragma("unroll") for( int k=0; k<10; k++ ) r.v[k] = p[k]; return r; }
__device__ __forceinline__ void stfe( i32 * p, fe const & f ) { _Pragma("unroll") for( int k=0; k<10; k++ ) p[k] = f.v[k]; }

template<int OP>
__global__ void __launch_bounds__(64)
k_probe( i32 const * __restrict__ in0, i32 const * __restrict__ in1, i32 const * __restrict__ aux, i32 * __restrict__ out ) {
  constexpr probe_shape_t S = probe_shape( OP );
  u32 const gt = blockIdx.x * 64u + threadIdx.x;
  u32 const c  = gt / (u32)S.lanes;
  int const ln = (int)(gt % (u32)S.lanes);
  i32 const * a = in0 + (size_t)c * S.s0;
  i32 const * b = in1 + (size_t)c * S.s1;
  i32 const * x = aux + (size_t)c * S.sa;
  i32       * o = out + (size_t)c * S.so;
  (void)b; (void)x; (void)ln;

  if constexpr( OP == P_MUL )       stfe( o, fe_mul( ldfe( a ), ldfe( b ) ) );
  if constexpr( OP == P_MUL_FOLD1 ) stfe( o, fe_mul_fold1( ldfe( a ), ldfe( b ) ) );
  if constexpr( OP == P_MUL_ONE )   stfe( o, fe_mul_one( ldfe( a ) ) );
  if constexpr( OP == P_SQN1 )      stfe( o, fe_sqn<1>( ldfe( a ) ) );
  if constexpr( OP == P_SQN2 )      stfe( o, fe_sqn<2>( ldfe( a ) ) );
  if constexpr( OP == P_SQ_FOLD )   stfe( o, fe_sq_fold( ldfe( a ) ) );
  if constexpr( OP >= P_MUL_FOLD2W_00 && OP <= P_MUL_FOLD2W_11 ) {
    fe r1, r2;
    fe_mul_fold2w< ((OP - P_MUL_FOLD2W_00) & 2) != 0, ((OP - P_MUL_FOLD2W_00) & 1) != 0 >
      ( r1, ldfe( a ), ldfe( b ), r2, ldfe( a + 10 ), ldfe( b + 10 ) );
    stfe( o, r1 ); stfe( o + 10, r2 );
  }
  if constexpr( OP >= P_SQ_FOLD2W_00 && OP <= P_SQ_FOLD2W_11 ) {
    fe r1, r2;
    fe_sq_fold2w< ((OP - P_SQ_FOLD2W_00) & 2) != 0, ((OP - P_SQ_FOLD2W_00) & 1) != 0 >( r1, ldfe( a ), r2, ldfe( a + 10 ) );
    stfe( o, r1 ); stfe( o + 10, r2 );
  }
  if constexpr( OP == P_MUL_HALF5 ) {
    half_t const H = half_ctx( (ln >> 2) & 1 );
    fe5 const m = fe_mul_half5( ldfe( a ), ldfe( b ), H );
    stfe( o + 10*ln, fe_join5( m ) );
  }
  if constexpr( OP == P_POW22523 )  stfe( o, fe_pow22523( ldfe( a ) ) );
  if constexpr( OP == P_FROMBYTES ) {
    u32 w[8]; _Pragma("unroll") for( int k=0; k<8; k++ ) w[k] = (u32)a[k];
    stfe( o, fe_frombytes( w ) );
  }
  if constexpr( OP == P_ISNONZERO )  o[0] = fe_isnonzero( ldfe( a ) ) ? 1 : 0;
  if constexpr( OP == P_ISNEGATIVE ) o[0] = fe_isnegative( ldfe( a ) );
  if constexpr( OP == P_SC_REDUCE ) {
    u32 w[16], r[8];
    _Pragma("unroll") for( int k=0; k<16; k++ ) w[k] = (u32)a[k];
    sc_reduce( r, w );
    _Pragma("unroll") for( int k=0; k<8; k++ ) o[k] = (i32)r[k];
  }
  if constexpr( OP == P_GE_DBL ) {
    p1p1 t = ge_dbl( ldfe( a ), ldfe( a + 10 ), ldfe( a + 20 ) );
    stfe( o, t.X ); stfe( o + 10, t.Y ); stfe( o + 20, t.Z ); stfe( o + 30, t.T );
  }
  if constexpr( OP == P_GE_P3 || OP == P_GE_P3_FOLD ) {
    p1p1 t; t.X = ldfe( a ); t.Y = ldfe( a + 10 ); t.Z = ldfe( a + 20 ); t.T = ldfe( a + 30 );
    p3 u = (OP == P_GE_P3) ? ge_p1p1_to_p3( t ) : ge_p1p1_to_p3_fold( t );
    stfe( o, u.X ); stfe( o + 10, u.Y ); stfe( o + 20, u.Z ); stfe( o + 30, u.T );
  }
  if constexpr( OP == P_GE_ADD || OP == P_GE_MADD ) {
    p3 u; u.X = ldfe( a ); u.Y = ldfe( a + 10 ); u.Z = ldfe( a + 20 ); u.T = ldfe( a + 30 );
    p1p1 t = ge_add< OP == P_GE_MADD >( u, ldfe( b ), ldfe( b + 10 ), ldfe( b + 20 ), ldfe( b + 30 ), x[0] != 0 );
    stfe( o, t.X ); stfe( o + 10, t.Y ); stfe( o + 20, t.Z ); stfe( o + 30, t.T );
  }
  if constexpr( OP == P_GE_TO_CACHED ) {
    p3 u; u.X = ldfe( a ); u.Y = ldfe( a + 10 ); u.Z = ldfe( a + 20 ); u.T = ldfe( a + 30 );
    fe cZ, cM, cP, cT;
    ge_to_cached( cZ, cM, cP, cT, u );
    stfe( o, cZ ); stfe( o + 10, cM ); stfe( o + 20, cP ); stfe( o + 30, cT );
  }
  if constexpr( OP == P_QUAD_P3 || OP == P_QUAD_BODY || OP == P_QUAD_CACHED_ROW ) {
    int const qd = ln & 3;
    u64 const m1 = __builtin_amdgcn_ballot_w64( qd & 1 ), m2 = __builtin_amdgcn_ballot_w64( qd & 2 );
    if constexpr( OP == P_QUAD_P3 ) {
      p1p1 t; t.X = ldfe( a ); t.Y = ldfe( a + 10 ); t.Z = ldfe( a + 20 ); t.T = ldfe( a + 30 );
      p3 u; quad_p3( u, t, m1, m2 );
      i32 * ol = o + 40*ln;
      stfe( ol, u.X ); stfe( ol + 10, u.Y ); stfe( ol + 20, u.Z ); stfe( ol + 30, u.T );
    } else if constexpr( OP == P_QUAD_BODY ) {
      p3 u; u.X = ldfe( a ); u.Y = ldfe( a + 10 ); u.Z = ldfe( a + 20 ); u.T = ldfe( a + 30 );
      u64 const mD = __builtin_amdgcn_ballot_w64( x[0] != 0 ), mN = __builtin_amdgcn_ballot_w64( x[1] != 0 );
      p1p1 t; quad_body( t, u, ldfe( b + 10*ln ), mD, mN, m1, m2 );
      i32 * ol = o + 40*ln;
      stfe( ol, t.X ); stfe( ol + 10, t.Y ); stfe( ol + 20, t.Z ); stfe( ol + 30, t.T );
    } else {
      p3 u; u.X = ldfe( a ); u.Y = ldfe( a + 10 ); u.Z = ldfe( a + 20 ); u.T = ldfe( a + 30 );
      stfe( o + 10*ln, quad_cached_row( u, m1, m2 ) );
    }
  }
  if constexpr( OP == P_QUAD_OWNC ) {
    int const qd = ln & 3;
    bool const isD = x[0] != 0, neg = x[1] != 0;
    u64 const mD = __builtin_amdgcn_ballot_w64( isD );
    fe C = ldfe( a + 10*qd );
    fe const pm = quad_p3_ownc( C );
    quad_body_ownc( C, pm, ldfe( b + 10*qd ), isD, neg, mD, qd );
    stfe( o + 10*qd, pm ); stfe( o + 40 + 10*qd, C );
  }
  if constexpr( OP == P_QUAD8_OWNC5 ) {
    int const qd = ln & 3;
    half_t const H = half_ctx( (ln >> 2) & 1 );
    bool const isD = x[0] != 0, neg = x[1] != 0;
    u64 const mD = __builtin_amdgcn_ballot_w64( isD );
    fe C = ldfe( a + 10*qd );
    fe5 const pm5 = quad8_p3_ownc5( C, H );
    fe const pm = fe_join5( pm5 );
    quad8_body_ownc5( C, pm5, ldfe( b + 10*qd ), isD, neg, mD, qd, H );
    stfe( o + 10*ln, pm ); stfe( o + 80 + 10*ln, C );
  }
  if constexpr( OP == P_SIGN_FE_INVERT ) stfe( o, fe_invert( ldfe( a ) ) );
  if constexpr( OP == P_SIGN_FE_TOBYTES ) {
    u32 w[8]; fe_tobytes_w( w, ldfe( a ) );
    _Pragma("unroll") for( int k=0; k<8; k++ ) o[k] = (i32)w[k];
  }
  if constexpr( OP == P_SIGN_RECODE ) {
    u32 s[8], dig[16];
    _Pragma("unroll") for( int k=0; k<8; k++ ) s[k] = (u32)a[k];
    recode_radix16( dig, s );
    _Pragma("unroll") for( int k=0; k<16; k++ ) o[k] = (i32)dig[k];
  }
  if constexpr( OP == P_SIGN_SCALARMULT_BASE ) {
    u32 s[8], enc[8];
    _Pragma("unroll") for( int k=0; k<8; k++ ) s[k] = (u32)a[k];
    scalarmult_base_enc( enc, s );
    _Pragma("unroll") for( int k=0; k<8; k++ ) o[k] = (i32)enc[k];
  }
  if constexpr( OP == P_SIGN_SC_MULADD ) {
    u32 kk[8], aa[8], rr[8], r[8];
    _Pragma("unroll") for( int k=0; k<8; k++ ) { kk[k] = (u32)a[k]; aa[k] = (u32)a[8+k]; rr[k] = (u32)b[k]; }
    sc_muladd( r, kk, aa, rr );
    _Pragma("unroll") for( int k=0; k<8; k++ ) o[k] = (i32)r[k];
  }
}

template<int OP>
static hipError_t
probe_launch( int op, unsigned blocks, i32 const * a, i32 const * b, i32 const * x, i32 * o ) {
  if constexpr( OP < P_OP_CNT ) {
    if( op != OP ) return probe_launch<OP + 1>( op, blocks, a, b, x, o );
    hipLaunchKernelGGL( k_probe<OP>, dim3( blocks ), dim3( 64 ), 0, 0, a, b, x, o );
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

extern "C" int          fd_probe_op_cnt( void ) { return P_OP_CNT; }
extern "C" char const * fd_probe_name( int op ) { return (op >= 0 && op < P_OP_CNT) ? probe_names[op] : NULL; }

extern "C" int
fd_probe_shape( int op, int * shape /* lanes, in0, in1, aux, out */ ) {
  if( op < 0 || op >= P_OP_CNT ) return -1;
  probe_shape_t S = probe_shape( op );
  shape[0] = S.lanes; shape[1] = S.s0; shape[2] = S.s1; shape[3] = S.sa; shape[4] = S.so;
  return 0;
}

/* Run probe `op` on n cases held in host arrays (case-major, the op's
   strides); 0 or the HIP error code. */
extern "C" int
fd_probe_run( int op, unsigned long n, int const * in0, int const * in1, int const * aux, int * out ) {
  if( op < 0 || op >= P_OP_CNT ) return (int)hipErrorInvalidValue;
  if( !n ) return 0;
  probe_shape_t S = probe_shape( op );
  unsigned long per = 64UL / (unsigned long)S.lanes;            /* cases per wave */
  unsigned long np  = (n + per - 1UL) / per * per;              /* padded with zero cases */
  if( np / per > 0x7fffffffUL ) return (int)hipErrorInvalidValue;
  size_t const sz[4] = { 4UL*np*(size_t)S.s0 + 4UL, 4UL*np*(size_t)S.s1 + 4UL, 4UL*np*(size_t)S.sa + 4UL, 4UL*np*(size_t)S.so + 4UL };
  void const * src[3] = { in0, in1, aux };
  int const    str[3] = { S.s0, S.s1, S.sa };
  void * d[4] = { NULL, NULL, NULL, NULL };
  hipError_t e = hipSuccess;
  for( int k=0; k<4 && e == hipSuccess; k++ ) {
    e = hipMalloc( &d[k], sz[k] );
    if( e == hipSuccess ) e = hipMemset( d[k], 0, sz[k] );
  }
  for( int k=0; k<3 && e == hipSuccess; k++ )
    if( str[k] ) e = src[k] ? hipMemcpy( d[k], src[k], 4UL*n*(size_t)str[k], hipMemcpyHostToDevice ) : hipErrorInvalidValue;
  if( e == hipSuccess ) e = probe_launch<0>( op, (unsigned)(np / per), (i32 const *)d[0], (i32 const *)d[1], (i32 const *)d[2], (i32 *)d[3] );
  if( e == hipSuccess ) e = hipDeviceSynchronize();
  if( e == hipSuccess ) e = hipMemcpy( out, d[3], 4UL*n*(size_t)S.so, hipMemcpyDeviceToHost );
  for( int k=0; k<4; k++ ) if( d[k] ) (void)hipFree( d[k] );
  return (int)e;
}
