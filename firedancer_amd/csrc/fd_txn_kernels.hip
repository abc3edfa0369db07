/* firedancer_amd/csrc/fd_txn_kernels.hip
 *
 * GPU transaction front end of the verify engine: parse a
 * batch of wire-format Solana transactions, one transaction per lane, with
 * the exact accept/reject behaviour and descriptor bytes of the reference's
 * fd_txn_parse (src/ballet/txn/fd_txn_parse.c:6-217; compact-u16 rules of
 * fd_compact_u16.h:35-87), and lay every signature of every well-formed
 * transaction out for the verify kernels: signature i of transaction t is
 * checked with account address i over the message payload[message_off, sz)
 * (fd_txn.h:159-217).  The message bytes are NOT copied: every signature of
 * a transaction points at the same bytes of the payload blob in HBM.
 *
 *   k_txn_parse   parse + signature layout (one lane per transaction)
 *   k_txn_reduce  per-transaction verdict: parse failure, else the first
 *                 failing signature's code in signature order, else 0
 *   k_desc_bsum, k_desc_bscan, k_desc_store
 *                 packed descriptors: a 64-bit exclusive scan of the
 *                 footprints and a second walk of the accepted payloads
 *                 that stores each descriptor at its offset
 *   k_desc_out    a chunk's offsets and packed bytes to mapped host memory
 *   k_txn_budget  (fd_txn_budget.h) per transaction its compute budget and fee
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fd_ed25519_kernels.h"

typedef uint8_t  u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int8_t   i8;

#include "fd_txn_dev.h"
#include "fd_txn_budget.h"   /* k_txn_budget: compiled here, behind fd_txn_dev.h */

using namespace fd_txn_dev;

namespace {

/* n bytes from an unaligned source as little-endian dwords */
__device__ __forceinline__ void
copy_dw( u32 * dst, u8 const * src, u32 ndw ) {
  for( u32 k=0u; k<ndw; k++ )
    dst[k] = (u32)src[4u*k] | ((u32)src[4u*k+1u] << 8) | ((u32)src[4u*k+2u] << 16) | ((u32)src[4u*k+3u] << 24);
}

} /* namespace */

__global__ void __launch_bounds__(64)
k_txn_parse( u32 txn_cnt, u8 const * __restrict__ payload, u32 const * __restrict__ toff, u32 const * __restrict__ tsz,
             u32 * __restrict__ fp_out, u8 * __restrict__ out, size_t out_stride, u32 const * __restrict__ tbase,
             u8 * __restrict__ pub, u8 * __restrict__ sig, u32 * __restrict__ moff, u32 * __restrict__ msz,
             i8 * __restrict__ skip ) {
  u32 t = blockIdx.x * 64u + threadIdx.x;
  if( t >= txn_cnt ) return;
  u8 const * p = payload + toff[t];
  u32 sz = tsz[t];
  u32 nsig = 0u, sig_off = 0u, acct_off = 0u, msg_off = 0u;
  /* no footprint reaches 2^32 - 1, so a wider stride bounds nothing */
  u32 cap = out_stride < 0xffffffffUL ? (u32)out_stride : 0xffffffffu;
  u32 fp = txn_parse( p, sz, out ? out + (size_t)t*out_stride : (u8 *)0, cap, &nsig, &sig_off, &acct_off, &msg_off );
  if( fp_out ) fp_out[t] = fp;
  if( !tbase ) return;
  u32 b = tbase[t], e = tbase[t+1u];
  if( !fp ) {                                 /* reserved slots of a rejected payload */
    for( u32 s=b; s<e; s++ ) skip[s] = (i8)TXN_ERR_PARSE;
    return;
  }
  /* host reserved payload[0] slots; a parsed transaction has exactly that
     many.  A caller-supplied tbase that reserved a different count (device
     API) rejects the transaction instead of verifying a subset: fail closed */
  if( e - b != nsig ) {
    if( fp_out ) fp_out[t] = 0u;
    for( u32 s=b; s<e; s++ ) skip[s] = (i8)TXN_ERR_PARSE;
    return;
  }
  for( u32 i=0u; i<nsig; i++ ) {
    u32 s = b + i;
    copy_dw( (u32 *)(pub + 32UL*s), p + acct_off + 32u*i,  8u );
    copy_dw( (u32 *)(sig + 64UL*s), p + sig_off  + 64u*i, 16u );
    moff[s] = toff[t] + msg_off;
    msz[s]  = sz - msg_off;
    skip[s] = 0;
  }
}

__global__ void __launch_bounds__(64)
k_txn_reduce( u32 txn_cnt, u32 const * __restrict__ fp, u32 const * __restrict__ tbase,
              i8 const * __restrict__ err, i8 * __restrict__ terr ) {
  u32 t = blockIdx.x * 64u + threadIdx.x;
  if( t >= txn_cnt ) return;
  if( !fp[t] ) { terr[t] = (i8)TXN_ERR_PARSE; return; }
  i8 r = 0;
  for( u32 s=tbase[t]; s<tbase[t+1u]; s++ ) { i8 e = err[s]; if( e ) { r = e; break; } }
  terr[t] = r;
}

/* Packed descriptors (fd_txn_dev.h, "packed descriptors"): three kernels,
   ordered by the stream alone. */

/* bsum[b] = the footprint total of transactions [64 b, 64 b + 64) */
__global__ void __launch_bounds__(64)
k_desc_bsum( u32 txn_cnt, u32 const * __restrict__ fp, u64 * __restrict__ bsum ) {
  u32 lane = threadIdx.x, t = blockIdx.x * TXN_PACK_BLOCK + lane;
  u32 incl = wave_scan_incl( t < txn_cnt ? fp[t] : 0u, lane );
  if( lane == 63u ) bsum[blockIdx.x] = (u64)incl;
}

/* One workgroup: bsum[0, nblk) becomes its own exclusive prefix sum, 64
   entries per turn of the loop, and *total the grand total (the descriptor
   pack's desc_off[txn_cnt]). */
__global__ void __launch_bounds__(64)
k_desc_bscan( u32 nblk, u64 * __restrict__ bsum, u64 * __restrict__ total ) {
  u32 lane = threadIdx.x;
  u64 carry = 0UL;
  for( u32 base=0u; base<nblk; base+=64u ) {          /* wave-uniform trip count */
    u32 i = base + lane;
    u32 v = i < nblk ? (u32)bsum[i] : 0u;
    u32 incl = wave_scan_incl( v, lane );
    if( i < nblk ) bsum[i] = carry + (u64)(incl - v);
    carry += (u64)(u32)__shfl( (int)incl, 63, 64 );
  }
  if( lane == 0u ) *total = carry;
}

/* desc_off[t] for every transaction, and the descriptor of every accepted
   one whose end is within cap */
__global__ void __launch_bounds__(64)
k_desc_store( u32 txn_cnt, u8 const * __restrict__ payload, u32 const * __restrict__ toff, u32 const * __restrict__ tsz,
              u32 const * __restrict__ fp, u64 const * __restrict__ bsum, u64 * __restrict__ desc_off,
              u8 * __restrict__ desc, u64 cap ) {
  u32 lane = threadIdx.x, t = blockIdx.x * TXN_PACK_BLOCK + lane;
  u32 f = t < txn_cnt ? fp[t] : 0u;
  u32 incl = wave_scan_incl( f, lane );
  if( t >= txn_cnt ) return;
  u64 off = bsum[blockIdx.x] + (u64)(incl - f);
  desc_off[t] = off;
  if( f && off + (u64)f <= cap ) txn_desc_store( payload + toff[t], tsz[t], desc + off, f );
}

/* A chunk's offsets and packed bytes, device -> mapped host memory, 16 B per
   lane: off[0 .. txn_cnt] and the first min( off[txn_cnt], cap ) bytes,
   rounded up to 16 (all four buffers are 16-aligned, and the byte buffers
   end on a multiple of 16 at or after cap).  The byte total is read from the scan's last element,
   so the host need not know it when it launches this. */
__global__ void __launch_bounds__(256)
k_desc_out( u8 * __restrict__ dst, u8 const * __restrict__ src, u64 * __restrict__ dst_off, u64 const * __restrict__ src_off,
            u32 txn_cnt, u64 cap ) {
  size_t i = (size_t)blockIdx.x * 256u + threadIdx.x, stride = (size_t)gridDim.x * 256u;
  u64 total = src_off[txn_cnt];
  size_t nv = (size_t)( ( ( total < cap ? total : cap ) + 15UL ) >> 4 );
  for( size_t k = i; k < nv; k += stride ) ((uint4 *)dst)[k] = ((uint4 const *)src)[k];
  size_t no = (size_t)txn_cnt + 1u, np = no >> 1;      /* the offsets two to a lane, the odd one last */
  for( size_t k = i; k < np; k += stride ) ((ulong2 *)dst_off)[k] = ((ulong2 const *)src_off)[k];
  if( (no & 1u) && i == 0 ) dst_off[no - 1u] = src_off[no - 1u];
}

/* The first two steps of the scan, for any plane of n u32 values whose every
   64-block sums below 2^32: d_bsum[b] = the sum of the blocks before block b,
   *d_total = the sum of all (n == 0: *d_total = 0 and nothing else). */
int
fd_amd_launch_scan64( uint32_t n, uint32_t const * d_val, uint64_t * d_bsum, uint64_t * d_total, hipStream_t stream ) {
  u32 nblk = (u32)( ( (u64)n + TXN_PACK_BLOCK - 1UL ) / TXN_PACK_BLOCK );
  if( nblk ) hipLaunchKernelGGL( k_desc_bsum, dim3(nblk), dim3(64), 0, stream, n, d_val, (u64 *)d_bsum );
  return fd_amd_launch_bscan64( nblk, d_bsum, d_total, stream );
}

/* The scan's second step alone, for a caller whose own kernel left the block
   totals: d_bsum[0, nblk) becomes its exclusive prefix sum, *d_total the sum. */
int
fd_amd_launch_bscan64( uint32_t nblk, uint64_t * d_bsum, uint64_t * d_total, hipStream_t stream ) {
  hipLaunchKernelGGL( k_desc_bscan, dim3(1), dim3(64), 0, stream, nblk, (u64 *)d_bsum, (u64 *)d_total );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int
fd_amd_launch_txn_pack( uint32_t txn_cnt, uint8_t const * d_payload, uint32_t const * d_toff, uint32_t const * d_tsz,
                        uint32_t const * d_fp, uint64_t * d_bsum, uint64_t * d_desc_off, uint8_t * d_desc,
                        uint64_t desc_cap, hipStream_t stream ) {
  u32 nblk = (u32)( ( (u64)txn_cnt + TXN_PACK_BLOCK - 1UL ) / TXN_PACK_BLOCK );
  if( fd_amd_launch_scan64( txn_cnt, d_fp, d_bsum, d_desc_off + txn_cnt, stream ) ) return -1;
  if( nblk ) hipLaunchKernelGGL( k_desc_store, dim3(nblk), dim3(64), 0, stream, txn_cnt, d_payload, d_toff, d_tsz, d_fp,
                                 (u64 const *)d_bsum, (u64 *)d_desc_off, d_desc, (u64)desc_cap );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int
fd_amd_launch_desc_out( void * d_dst_mapped, uint8_t const * d_desc, void * d_off_mapped, uint64_t const * d_desc_off,
                        uint32_t txn_cnt, uint64_t cap, uint64_t bound, hipStream_t stream ) {
  /* the grid covers the larger of the offsets and the chunk's bound (the
     real total is at most that), one 16-B word per lane and turn */
  uint64_t words = ( ( bound < cap ? bound : cap ) + 15UL ) >> 4;
  if( words < (uint64_t)txn_cnt + 1UL ) words = (uint64_t)txn_cnt + 1UL;
  uint64_t nb = ( words + 255UL ) / 256UL;
  if( nb > 1024UL ) nb = 1024UL;
  hipLaunchKernelGGL( k_desc_out, dim3((unsigned)nb), dim3(256), 0, stream, (u8 *)d_dst_mapped, d_desc, (u64 *)d_off_mapped,
                      (u64 const *)d_desc_off, txn_cnt, (u64)cap );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int
fd_amd_launch_txn_parse( uint32_t txn_cnt, uint8_t const * d_payload, uint32_t const * d_toff,
                         uint32_t const * d_tsz, uint32_t * d_fp, uint8_t * d_out, size_t out_stride,
                         uint32_t const * d_tbase, uint8_t * d_pub, uint8_t * d_sig, uint32_t * d_off,
                         uint32_t * d_sz, int8_t * d_skip, hipStream_t stream ) {
  if( !txn_cnt ) return 0;
  hipLaunchKernelGGL( k_txn_parse, dim3((txn_cnt + 63u)/64u), dim3(64), 0, stream, txn_cnt, d_payload, d_toff, d_tsz,
                      d_fp, d_out, out_stride, d_tbase, d_pub, d_sig, d_off, d_sz, d_skip );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int
fd_amd_launch_txn_reduce( uint32_t txn_cnt, uint32_t const * d_fp, uint32_t const * d_tbase,
                          int8_t const * d_err, int8_t * d_terr, hipStream_t stream ) {
  if( !txn_cnt ) return 0;
  hipLaunchKernelGGL( k_txn_reduce, dim3((txn_cnt + 63u)/64u), dim3(64), 0, stream, txn_cnt, d_fp, d_tbase, d_err, d_terr );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
