/* firedancer_amd/csrc/fd_ed25519_window.h -- dedup across submissions: a
   device-resident window of the last `depth` tags a caller published
   (include/fd_ed25519_amd.h, "The dedup window").  Included by
   fd_ed25519_kernels.hip only, behind fd_ed25519_keep.h, whose launch calls
   win_launch_step at the end of this file.

   The window's state, one device allocation (fd_amd_win_layout):

     ring[depth]  u64: the tag of insertion q sits at ring[q % depth]
     head[2]      u64: H, the number of tags ever inserted.  Two words taken
                  in turn: submission number s of the window (the host counts
                  them) reads head[s & 1] and leaves H for the next one in the
                  other word, so no kernel has to wait for every lane that
                  still reads the old value
     key[cap]     u64, stamp[cap] u64: an open-addressed map, linear probing,
                  cap a power of two >= 4 depth, home slot keep_home( tag,
                  window salt, cap - 1 ).  key 0 = empty; stamp = q + 1 of the
                  key's latest insertion.

   Nothing is ever deleted from the map.  A key is live iff its stamp is
   nonzero and stamp - 1 + depth >= H; a tag that is offered again after it
   expired finds its old slot and raises the stamp.  Expired keys go when the
   host asks for a REBUILD ahead of a submission: k_win_clear empties the map
   and k_win_rebuild re-enters the live range of the ring with its stamps.
   The host asks whenever the items offered since the last rebuild, this
   submission's included, exceed depth; so the map holds at most depth keys
   after a rebuild and at most depth more before the next, 2 depth <= cap / 2
   in all, and every probe ends at an empty slot.  All the same every probe
   loop is bounded by cap: no contents can make a lane spin.

   One submission of n <= depth items, the kernels ordered by the stream, no
   workgroup ever waiting for another:

     k_keep_clear / k_keep_insert / k_keep_mark      the in-batch rule: flag[]
   - the wait for the previous submission's window step (another stream's) -
     ( k_win_clear, k_win_rebuild           when the host asked )
     k_win_query    a flagged item whose nonzero tag is live in the window, as
                    the window stood when the submission started, loses its
                    flag (and its masked footprint); flag2[i] = flag[i] and
                    tag[i] != 0: the items the window takes in; and per 64
                    items their number
     k_win_scan     those block totals' prefix sums, one workgroup: the
                    insertion rank r of every taken item; H + their count
                    into the other head word
     k_win_insert   ring[(H + r) % depth] = tag; the key claimed or found,
                    its stamp raised to H + r + 1
   - the event the next submission waits for -
     the scan of flag, k_keep_store                  keep[], keep_cnt

   Only the three kernels between the two marks are ordered among
   submissions; they are as few and as small as the rule allows, because with
   several submissions in flight that stretch is serial.

   k_win_query reads H, keys and stamps with plain loads: everything it looks
   at was written by kernels that finished before it started (the stream's
   order within a submission, the window's event between two submissions'
   streams), and a kernel boundary makes those stores visible.  Inside
   k_win_insert and k_win_rebuild a key is looked at only through the value
   its agent-scope compare-and-swap returns, and a stamp only raised by an
   agent-scope atomic max, for the reason given in fd_ed25519_keep.h: the
   workgroups of one launch sit on eight XCDs with an L2 each.

   Why the rule queries the window as of the submission's start, and not item
   by item as FD_TCACHE_INSERT would: item by item, whether item i evicts the
   oldest tag depends on how many items before i survived, a serial chain
   through the batch.  As of the start, every item's answer is independent;
   the only cost is that a tag this submission's own inserts push out still
   counts as seen inside it (the header states the exact relation). */
#ifndef FD_ED25519_WINDOW_H
#define FD_ED25519_WINDOW_H

__global__ void __launch_bounds__(256)
k_win_clear( u64 * __restrict__ key, u64 * __restrict__ stamp, u32 cap ) {
  u32 s = blockIdx.x * 256u + threadIdx.x;
  if( s >= cap ) return;
  key[s] = 0UL; stamp[s] = 0UL;
}

/* Claim or find t's slot and raise its stamp to st.  A lane that runs out of
   trips enters nothing: the tag is then simply not remembered by the map. */
__device__ __forceinline__ void
win_enter( u64 t, u64 st, u64 * __restrict__ key, u64 * __restrict__ stamp, u32 cap, u64 salt ) {
  u32 const mask = cap - 1u;
  u32 s = keep_home( t, salt, mask );
  for( u32 trip=0u; trip<cap; trip++ ) {
    unsigned long long seen = 0ULL;
    bool won = __hip_atomic_compare_exchange_strong( (unsigned long long *)(key + s), &seen, (unsigned long long)t,
                                                     __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
    if( won || seen == (unsigned long long)t ) {
      (void)__hip_atomic_fetch_max( (unsigned long long *)(stamp + s), (unsigned long long)st, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT );
      return;
    }
    s = (s + 1u) & mask;
  }
}

/* Ring position p holds insertion q, the one q in [max( 0, H - depth ), H)
   with q % depth == p (none while H <= p).  A zero entry (never written by
   an insert; import refuses it) is skipped. */
__global__ void __launch_bounds__(256)
k_win_rebuild( u64 const * __restrict__ ring, u64 const * __restrict__ head /* the current word */, u64 depth,
               u64 * __restrict__ key, u64 * __restrict__ stamp, u32 cap, u64 salt ) {
  u64 p = (u64)blockIdx.x * 256UL + threadIdx.x;
  if( p >= depth ) return;
  u64 const H = *head;
  u64 q = p;
  if( H <= depth ) { if( p >= H ) return; }
  else { u64 const b = H - depth; q = b + ( p + depth - b % depth ) % depth; }
  u64 const t = ring[p];
  if( !t ) return;
  win_enter( t, q + 1UL, key, stamp, cap, salt );
}

/* fpk: the masked footprint plane of the transaction form (NULL: the
   signature form).  A lane that runs out of trips drops its item: fail
   closed, as in k_keep_mark.  One wave per 64 items, as the scan's kernels:
   bsum2[b] = the taken items of block b. */
__global__ void __launch_bounds__(64)
k_win_query( u32 n, u64 const * __restrict__ tag, u32 * __restrict__ flag, u32 * __restrict__ flag2, u64 * __restrict__ bsum2,
             u32 * __restrict__ fpk, u64 const * __restrict__ key, u64 const * __restrict__ stamp, u32 cap, u64 salt,
             u64 const * __restrict__ head, u64 depth ) {
  u32 lane = threadIdx.x, i = blockIdx.x * TXN_PACK_BLOCK + lane;
  u64 const t = i < n ? tag[i] : 0UL;
  u32 f2 = 0u;
  if( i < n && flag[i] && t ) {
    u64 const H = *head;
    u32 const mask = cap - 1u;
    u32 s = keep_home( t, salt, mask );
    bool live = true;
    for( u32 trip=0u; trip<cap; trip++ ) {
      u64 const k = key[s];
      if( k == t ) { u64 const st = stamp[s]; live = st && st - 1UL + depth >= H; break; }
      if( !k ) { live = false; break; }
      s = (s + 1u) & mask;
    }
    if( live ) { flag[i] = 0u; if( fpk ) fpk[i] = 0u; }
    else f2 = 1u;
  }
  if( i < n ) flag2[i] = f2;
  u32 incl = fd_txn_dev::wave_scan_incl( f2, lane );
  if( lane == 63u ) bsum2[blockIdx.x] = (u64)incl;
}

/* One workgroup (k_desc_bscan's loop): bsum2[0, nblk) becomes its own
   exclusive prefix sum, and the other head word H + the grand total. */
__global__ void __launch_bounds__(64)
k_win_scan( u32 nblk, u64 * __restrict__ bsum2, u64 const * __restrict__ head, u64 * __restrict__ head_next ) {
  u32 lane = threadIdx.x;
  u64 carry = 0UL;
  for( u32 base=0u; base<nblk; base+=64u ) {          /* wave-uniform trip count */
    u32 i = base + lane;
    u32 v = i < nblk ? (u32)bsum2[i] : 0u;
    u32 incl = fd_txn_dev::wave_scan_incl( v, lane );
    if( i < nblk ) bsum2[i] = carry + (u64)(incl - v);
    carry += (u64)(u32)__shfl( (int)incl, 63, 64 );
  }
  if( lane == 0u ) *head_next = *head + carry;
}

/* per 64-item block, as k_keep_store: the in-wave scan of flag2 on top of the
   block's base is the item's insertion rank */
__global__ void __launch_bounds__(64)
k_win_insert( u32 n, u64 const * __restrict__ tag, u32 const * __restrict__ flag2, u64 const * __restrict__ bsum2,
              u64 * __restrict__ ring, u64 const * __restrict__ head, u64 depth, u64 * __restrict__ key,
              u64 * __restrict__ stamp, u32 cap, u64 salt ) {
  u32 lane = threadIdx.x, i = blockIdx.x * TXN_PACK_BLOCK + lane;
  u32 f = i < n ? flag2[i] : 0u;
  u32 incl = fd_txn_dev::wave_scan_incl( f, lane );
  if( !f ) return;
  u64 const q = *head + bsum2[blockIdx.x] + (u64)(incl - 1u);   /* the word this submission reads: nobody writes it now */
  u64 const t = tag[i];
  ring[q % depth] = t;                                          /* the rank is below n <= depth: no two lanes share a position */
  win_enter( t, q + 1UL, key, stamp, cap, salt );
}

fd_amd_win_layout_t
fd_amd_win_layout( size_t depth ) {
  fd_amd_win_layout_t L;
  size_t cap = 256UL, o = 0;
  while( cap < 4UL*depth ) cap <<= 1;
  L.cap   = cap;
  L.ring  = o; o = ( o + 8UL*( depth ? depth : 1UL ) + 255UL ) & ~(size_t)255UL;
  L.head  = o; o += 256UL;
  L.key   = o; o += 8UL*cap;
  L.stamp = o; o += 8UL*cap;
  L.total = o;
  return L;
}

fd_amd_win_scratch_t
fd_amd_win_scratch( size_t n ) {
  fd_amd_win_scratch_t S;
  size_t nblk = ( n + TXN_PACK_BLOCK - 1UL ) / TXN_PACK_BLOCK, o = fd_amd_keep_layout( n ).total;
  S.flag2 = o; o = ( o + 4UL*( n ? n : 1UL ) + 255UL ) & ~(size_t)255UL;
  S.bsum2 = o; o = ( o + 8UL*( nblk ? nblk : 1UL ) + 255UL ) & ~(size_t)255UL;
  S.total = o;
  return S;
}

int
fd_amd_launch_win_rebuild( fd_amd_win_dev_t const * w, hipStream_t stream ) {
  hipLaunchKernelGGL( k_win_clear,   dim3(w->cap/256u), dim3(256), 0, stream, (u64 *)w->key, (u64 *)w->stamp, w->cap );
  hipLaunchKernelGGL( k_win_rebuild, dim3((unsigned)((w->depth + 255UL)/256UL)), dim3(256), 0, stream, (u64 const *)w->ring,
                      (u64 const *)w->head + w->cur, (u64)w->depth, (u64 *)w->key, (u64 *)w->stamp, w->cap, (u64)w->salt );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* The window's part of fd_amd_launch_keep_win (fd_ed25519_keep.h), n > 0,
   behind k_keep_mark: the stretch that is ordered among submissions, between
   the wait for the event of the one before and the event of this one. */
static int
win_launch_step( fd_amd_win_dev_t const * w, u32 n, u64 const * tag, u32 * flag, u32 * flag2, u64 * bsum2, u32 * fpk,
                 hipStream_t stream ) {
  u32 const nblk = (n + TXN_PACK_BLOCK - 1u)/TXN_PACK_BLOCK;
  u64 const * head = (u64 const *)w->head + w->cur;
  if( w->wait && hipStreamWaitEvent( stream, w->wait, 0 ) != hipSuccess ) return -1;
  if( w->rebuild && fd_amd_launch_win_rebuild( w, stream ) ) return -1;
  hipLaunchKernelGGL( k_win_query, dim3(nblk), dim3(64), 0, stream, n, tag, flag, flag2, bsum2, fpk, (u64 const *)w->key,
                      (u64 const *)w->stamp, w->cap, (u64)w->salt, head, (u64)w->depth );
  hipLaunchKernelGGL( k_win_scan, dim3(1), dim3(64), 0, stream, nblk, bsum2, head, (u64 *)w->head + ( w->cur ^ 1u ) );
  hipLaunchKernelGGL( k_win_insert, dim3(nblk), dim3(64), 0, stream, n, tag, (u32 const *)flag2, (u64 const *)bsum2,
                      (u64 *)w->ring, head, (u64)w->depth, (u64 *)w->key, (u64 *)w->stamp, w->cap, (u64)w->salt );
  if( hipGetLastError() != hipSuccess ) return -1;
  if( w->done && hipEventRecord( w->done, stream ) != hipSuccess ) return -1;
  return 0;
}

#endif /* FD_ED25519_WINDOW_H */
