/* firedancer_amd/csrc/fd_ed25519_keep.h -- the publish list of a batch: the
   ascending indices of the items that verified and are the first of their
   dedup tag (include/fd_ed25519_amd.h, "Survivors").  Included by
   fd_ed25519_kernels.hip only.

   Item i of n, with verdict err[i] and tag tag[i], is a survivor iff
   err[i] == 0 and ( tag[i] == 0 or no j < i has err[j] == 0 and
   tag[j] == tag[i] ).  Kernels ordered by the stream; no workgroup ever waits
   for another:

     k_keep_clear   the table: every key 0 (empty), every index ~0
     k_keep_insert  every passing item with a nonzero tag claims or finds its
                    key and lowers the slot's index to its own
     k_keep_mark    flag[i] = passing and ( tag 0 or the slot's index is i );
                    the transaction form also masks the footprint plane
     the scan of the flags (fd_amd_launch_scan64: the descriptor scan's block
                    totals and one-workgroup loop, fd_txn_kernels.hip)
     k_keep_store   keep[rank] = i for every flagged item

   The table is open-addressed in global memory, linear probing, capacity a
   power of two >= 2 n: a u64 key plane (the tag itself; 0 = empty) and a u32
   index plane.  The home slot is a 64-bit mixer of tag ^ salt: tags are
   hashes an attacker chooses, and with a known slot function it could grind
   tags into one probe chain and make the insert quadratic; the salt is a
   secret of the caller (the engine draws it from the OS).  The outputs do not
   depend on it.

   Inside k_keep_insert a key is only ever looked at through the value its
   agent-scope compare-and-swap returns: the workgroups of one launch run on
   eight XCDs with an L2 each, and a plain load of a key another XCD has just
   claimed may be served from this XCD's stale line; it would then read
   "empty" or an old key and walk past the item's own slot.  The atomic is
   performed where all XCDs meet, so its return value is the key's current
   value.  k_keep_mark runs behind the insert kernel's boundary, which makes
   every store of the launch before it visible: plain loads there. */
#ifndef FD_ED25519_KEEP_H
#define FD_ED25519_KEEP_H

#define KEEP_EMPTY_IDX 0xffffffffu

/* splitmix64's finalizer: every input bit reaches every output bit */
__device__ __forceinline__ u32
keep_home( u64 tag, u64 salt, u32 mask ) {
  u64 x = tag ^ salt;
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9UL;
  x ^= x >> 27; x *= 0x94d049bb133111ebUL;
  x ^= x >> 31;
  return (u32)x & mask;
}

__global__ void __launch_bounds__(256)
k_keep_clear( u64 * __restrict__ key, u32 * __restrict__ idx, u32 cap ) {
  u32 s = blockIdx.x * 256u + threadIdx.x;
  if( s >= cap ) return;
  key[s] = 0UL; idx[s] = KEEP_EMPTY_IDX;
}

/* cap slots, mask = cap - 1; cap >= 2 n, so an empty slot always ends a
   probe.  The loop is bounded by cap all the same (k_dsmp's step guard): no
   table contents, a stale scratch included, can make a lane spin.  A lane
   that runs out of trips inserts nothing and k_keep_mark, finding no key,
   drops the item: fail closed. */
__global__ void __launch_bounds__(256)
k_keep_insert( u32 n, i8 const * __restrict__ err, u64 const * __restrict__ tag, u64 * __restrict__ key,
               u32 * __restrict__ idx, u32 cap, u64 salt ) {
  u32 i = blockIdx.x * 256u + threadIdx.x;
  if( i >= n || err[i] ) return;
  u64 const t = tag[i];
  if( !t ) return;
  u32 const mask = cap - 1u;
  u32 s = keep_home( t, salt, mask );
  for( u32 trip=0u; trip<cap; trip++ ) {
    unsigned long long seen = 0ULL;
    bool won = __hip_atomic_compare_exchange_strong( (unsigned long long *)(key + s), &seen, (unsigned long long)t,
                                                     __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
    if( won || seen == (unsigned long long)t ) {   /* claimed it, or another item of this tag had */
      (void)__hip_atomic_fetch_min( idx + s, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
      return;
    }
    s = (s + 1u) & mask;
  }
}

/* fp / fpk (NULL: the signature form): fpk[i] = flag ? fp[i] : 0, the
   footprint plane the descriptor pack then runs on */
__global__ void __launch_bounds__(256)
k_keep_mark( u32 n, i8 const * __restrict__ err, u64 const * __restrict__ tag, u64 const * __restrict__ key,
             u32 const * __restrict__ idx, u32 cap, u64 salt, u32 * __restrict__ flag, u32 const * __restrict__ fp,
             u32 * __restrict__ fpk ) {
  u32 i = blockIdx.x * 256u + threadIdx.x;
  if( i >= n ) return;
  u32 f = 0u;
  if( !err[i] ) {
    u64 const t = tag[i];
    if( !t ) f = 1u;
    else {
      u32 const mask = cap - 1u;
      u32 s = keep_home( t, salt, mask );
      for( u32 trip=0u; trip<cap; trip++ ) {
        u64 const k = key[s];
        if( k == t ) { f = idx[s] == i ? 1u : 0u; break; }
        if( !k ) break;
        s = (s + 1u) & mask;
      }
    }
  }
  flag[i] = f;
  if( fpk ) fpk[i] = f ? fp[i] : 0u;
}

/* per 64-item block the in-wave scan of the flags on top of the block's base
   (bsum, after the one-workgroup loop): a flagged item's rank */
__global__ void __launch_bounds__(64)
k_keep_store( u32 n, u32 const * __restrict__ flag, u64 const * __restrict__ bsum, u32 * __restrict__ keep ) {
  u32 lane = threadIdx.x, i = blockIdx.x * TXN_PACK_BLOCK + lane;
  u32 f = i < n ? flag[i] : 0u;
  u32 incl = fd_txn_dev::wave_scan_incl( f, lane );
  if( f ) keep[ bsum[blockIdx.x] + (u64)(incl - 1u) ] = i;
}

fd_amd_keep_layout_t
fd_amd_keep_layout( size_t n ) {
  fd_amd_keep_layout_t L;
  size_t cap = 64UL;
  while( cap < 2UL*n ) cap <<= 1;
  size_t nblk = ( n + TXN_PACK_BLOCK - 1UL ) / TXN_PACK_BLOCK, o = 0;
  L.cap  = cap;
  L.key  = o; o = ( o + 8UL*cap + 255UL ) & ~(size_t)255UL;
  L.idx  = o; o = ( o + 4UL*cap + 255UL ) & ~(size_t)255UL;
  L.flag = o; o = ( o + 4UL*( n ? n : 1UL ) + 255UL ) & ~(size_t)255UL;
  L.bsum = o; o = ( o + 8UL*( nblk ? nblk : 1UL ) + 255UL ) & ~(size_t)255UL;
  L.total = o;
  return L;
}

/* the window's stages (fd_ed25519_window.h, included behind this file) */
static int win_launch_step( fd_amd_win_dev_t const * w, u32 n, u64 const * tag, u32 * flag, u32 * flag2, u64 * bsum2, u32 * fpk,
                            hipStream_t stream );

int
fd_amd_launch_keep( uint32_t n, int8_t const * d_err, uint64_t const * d_tag, uint32_t const * d_fp, uint32_t * d_fpk,
                    uint32_t * d_keep, uint64_t * d_keep_cnt, void * d_scratch, uint64_t salt, hipStream_t stream ) {
  return fd_amd_launch_keep_win( n, d_err, d_tag, d_fp, d_fpk, d_keep, d_keep_cnt, d_scratch, salt, NULL, stream );
}

/* w == NULL: the launches above and nothing else.  With a window, and n > 0,
   its step goes between k_keep_mark and the scan; the scratch is then
   fd_amd_win_scratch( n ). */
int
fd_amd_launch_keep_win( uint32_t n, int8_t const * d_err, uint64_t const * d_tag, uint32_t const * d_fp, uint32_t * d_fpk,
                        uint32_t * d_keep, uint64_t * d_keep_cnt, void * d_scratch, uint64_t salt,
                        fd_amd_win_dev_t const * w, hipStream_t stream ) {
  if( n > FD_AMD_KEEP_MAX || ( w && (uint64_t)n > w->depth ) ) return -1;
  fd_amd_keep_layout_t L = fd_amd_keep_layout( n );
  fd_amd_win_scratch_t S = fd_amd_win_scratch( n );
  u8 * w8 = (u8 *)d_scratch;
  u64 * key = (u64 *)(w8 + L.key), * bsum = (u64 *)(w8 + L.bsum);
  u32 * idx = (u32 *)(w8 + L.idx), * flag = (u32 *)(w8 + L.flag);
  u32 const cap = (u32)L.cap;
  if( n ) {
    hipLaunchKernelGGL( k_keep_clear,  dim3(cap/256u ? cap/256u : 1u), dim3(256), 0, stream, key, idx, cap );
    hipLaunchKernelGGL( k_keep_insert, dim3((n + 255u)/256u), dim3(256), 0, stream, n, d_err, (u64 const *)d_tag, key, idx, cap, (u64)salt );
    hipLaunchKernelGGL( k_keep_mark,   dim3((n + 255u)/256u), dim3(256), 0, stream, n, d_err, (u64 const *)d_tag, (u64 const *)key,
                        (u32 const *)idx, cap, (u64)salt, flag, d_fp, d_fpk );
    if( w && win_launch_step( w, n, (u64 const *)d_tag, flag, (u32 *)(w8 + S.flag2), (u64 *)(w8 + S.bsum2), d_fpk, stream ) ) return -1;
  }
  if( fd_amd_launch_scan64( n, flag, bsum, d_keep_cnt, stream ) ) return -1;   /* n == 0: *d_keep_cnt = 0 and nothing else */
  if( n ) hipLaunchKernelGGL( k_keep_store, dim3((n + TXN_PACK_BLOCK - 1u)/TXN_PACK_BLOCK), dim3(64), 0, stream, n, (u32 const *)flag,
                              (u64 const *)bsum, d_keep );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

#endif /* FD_ED25519_KEEP_H */
