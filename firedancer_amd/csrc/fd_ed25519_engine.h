/* firedancer_amd/csrc/fd_ed25519_engine.h -- internal: the batch engine's
   slots (one chunk in flight each; driven by fd_ed25519_engine.cpp alone: by
   run_ring for the synchronous calls, one at a time by the submit calls),
   the argument checks the multi-device engine shares with it, the NUMA
   helpers (fd_numa.cpp) and the transaction slot rule (fd_amd_txn_slots1,
   also the streaming tile's). */
#ifndef FD_ED25519_ENGINE_H
#define FD_ED25519_ENGINE_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fd_ed25519_amd.h"
#include "../../include/fd_txn_amd.h"   /* fd_txn_amd_budget_t */

/* The chunk in flight on a slot: what slot_drain delivers to the caller once
   the slot's event has fired, written by the two launch tails
   (slot_launch_sig, slot_launch_txn_dev) and cleared by slot_forget alone. */
struct slot_flight_t {
  /* verdicts and tags: the first ncp of cp[], each `sz` bytes from the slot's
     mapped staging (h_err, h_terr, h_tag, h_ttag, h_budget) to the caller's array */
  struct { void * dst; void const * src; ulong sz; } cp[5];
  int     ncp;
  ulong   chk_err, chk_terr;   /* verdict bytes the launch writes to h_err / h_terr (checked for FD_AMD_VERDICT_DEVICE) */
  /* descriptors (do_out NULL: not asked for): on delivery
     do_out[0 .. do_n] = *d_base + h_doff[..] (do_n: the chunk's transactions),
     the h_doff[do_n] bytes go to d_out + *d_base (d_cap: the caller's
     capacity) and *d_base grows by them -- so chunks must be drained in the
     order they were launched */
  ulong * do_out; ulong do_n;
  uchar * d_out;  ulong d_cap;
  ulong * d_base;
  /* survivors (k_out NULL: not asked for): on delivery *k_cnt = h_kcnt[0],
     at most k_n, and that many entries of h_keep go to k_out */
  uint *  k_out;  ulong * k_cnt;  ulong k_n;
  /* output frames (e_off NULL: not asked for; else k_out is set): on delivery
     h_eoff[0 .. count] go to e_off and h_esz[0 .. count) to e_sz, count being
     the survivors'; e_cap: the extent's capacity, which h_eoff[count] never
     exceeds */
  ulong * e_off;  uint * e_sz;  ulong e_cap;
};

/* The emit arguments of a submission, checked (fd_ed25519_engine.cpp,
   emit_args_check): out == NULL: none; dev: out's device address, from the
   registration table. */
struct emit_args_t { void * out; ulong cap; ulong * off; uint * sz; uint64_t dev; };

struct slot_t {
  /* device */
  uint8_t  * d_pub;  uint8_t * d_sig; uint8_t * d_blob;
  uint32_t * d_off;  uint32_t * d_sz; int8_t * d_err; void * d_ws;
  /* pinned host staging */
  uint8_t  * h_blob; int8_t * h_err;
  hipStream_t stream;
  hipEvent_t  done;
  uint8_t  * d_pack; uint8_t * h_pack;   /* packed [pub|sig|off|sz|blob] for n: one H2D per chunk */
  uint8_t  * m_pack;                     /* device address of the mapped h_pack (latency path reads it in place) */
  void * m_err, * m_terr;   /* device addresses of the mapped h_err / h_terr */
  int        strict;     /* the owning engine's mode (fd_ed25519_amd_set_mode): 1 = its launches add k_strict */
  int        busy;       /* a chunk is in flight: `fl` says where its outputs go */
  slot_flight_t fl;
  /* transaction front end (allocated on first use): per-transaction
     payload offset/size, footprint, signature-slot base, verdict; per-slot
     skip plane */
  uint32_t * d_toff; uint32_t * d_tsz; uint32_t * d_fp; uint32_t * d_tbase; int8_t * d_terr; int8_t * d_skip;
  uint32_t * h_toff; uint32_t * h_tsz; uint32_t * h_tbase; int8_t * h_terr;
  /* dedup tags (allocated by the first call that asks for them): one mapped
     pinned buffer, h_tag[cap] for per-signature tags and h_ttag[cap] behind
     it for per-transaction tags, both written in place by k_tag_out /
     k_tag_gather; m_tag / m_ttag: their device addresses */
  ulong * h_tag;  ulong * h_ttag;
  void  * m_tag;  void  * m_ttag;
  /* packed descriptors (allocated by the first call that asks for them).
     d_dpack, one device allocation: d_doff[cap+1], the chunk-relative 64-bit
     offsets; d_dbsum, the scan's block totals; d_desc[desc_stage], the packed
     bytes.  h_dpack, one mapped pinned allocation written by k_desc_out:
     h_doff[cap+1] and h_desc[desc_stage] (m_doff / m_desc: their device
     addresses).  desc_stage: a chunk's worst case, a multiple of 256. */
  uint8_t * d_dpack; ulong * d_doff; ulong * d_dbsum; uint8_t * d_desc;
  uint8_t * h_dpack; ulong * h_doff; uint8_t * h_desc;
  void    * m_doff;  void  * m_desc;
  ulong     desc_stage;
  /* survivors (fd_ed25519_amd_submit_*_keep; allocated by the first
     submission that asks for them).  d_kpack, one device allocation:
     d_kscr, the filter's scratch (fd_amd_keep_layout( cap )); d_ktag[cap],
     the per-transaction tags gathered on the device; d_fpk[cap], the
     footprint plane masked by the filter, which the descriptor pack then
     runs on.  h_kpack, one mapped pinned allocation the filter's kernels
     write: h_kcnt, the count, on a 256-byte line, and h_keep[cap] behind it
     (m_kcnt / m_keep: their device addresses).  salt: the owning engine's.
     keep_arm / kcnt_arm: the launch under way is a _keep submission, so the
     slot's launch tail adds the filter and the drain delivers to them (set
     and cleared by submit_run, as tick_arm). */
  uint8_t * d_kpack; void * d_kscr; ulong * d_ktag; uint32_t * d_fpk;
  uint8_t * h_kpack; ulong * h_kcnt; uint * h_keep;
  void    * m_kcnt;  void  * m_keep;
  ulong     salt;
  uint    * keep_arm; ulong * kcnt_arm;
  /* output frames (fd_ed25519_amd_submit_*_emit; allocated by the first
     submission that asks for them).  d_epack, one device allocation: the emit
     kernels' scratch (fd_amd_emit_layout( cap )).  h_epack, one mapped pinned
     allocation the kernels write: h_eoff[cap+1] and h_esz[cap] behind it
     (m_eoff / m_esz: their device addresses).  emit_arm: the launch under way
     is an _emit submission (out != NULL), so the slot's launch tail adds the
     emit step behind the filter (set and cleared by submit_run, as keep_arm). */
  uint8_t * d_epack;
  uint8_t * h_epack; ulong * h_eoff; uint * h_esz;
  void    * m_eoff;  void  * m_esz;
  emit_args_t emit_arm;
  /* frag submissions (fd_ed25519_amd_submit_frags; allocated by the first
     one).  d_fpack, one device allocation: the idle block, 96 zero bytes on a
     256-byte line, which the records of items without a frag point at, and
     d_fstat[cap] behind it, the items' statuses (k_frag_list writes them,
     k_frag_verdict reads them).  frag_arm: the launch under way is a frag
     submission (mcache != NULL: its lines' device address), so the slot's
     launch tail puts k_frag_verdict behind the verify kernels (set and
     cleared by stage_frags). */
  uint8_t * d_fpack; int8_t * d_fstat;
  struct { void const * mcache; ulong depth, seq0; } frag_arm;
  /* compute budget (the _budget calls; allocated by the first call that asks
     for it): h_budget[cap], fd_txn_amd_budget_t records in mapped pinned
     memory that k_txn_budget writes in place (m_budget: its device address) */
  fd_txn_amd_budget_t * h_budget; void * m_budget;
  /* the dedup window (fd_ed25519_amd_set_window): win_arm, the engine's
     window while a _keep submission is being launched (NULL: none attached),
     so the filter step runs against it; win_done, recorded behind that step
     (created with the survivor buffers): the next _keep submission's stream,
     on whichever slot, waits for it ahead of its own filter step */
  fd_ed25519_amd_window_t * win_arm;
  hipEvent_t win_done;
  /* asynchronous submissions (fd_ed25519_amd_submit_*): the ticket the slot
     carries; its completion word, 8 bytes on a 64-byte line of their own in
     mapped coherent pinned memory, to which k_ticket stores that ticket behind
     the chunk's kernels (m_tick: its device address); tick_arm: the launch
     under way is a submission that polls the word, so the slot's launch ends
     with k_ticket; a_dbase: the descriptor byte base of a submission (always 0:
     it is one chunk), what fl.d_base points at */
  ulong   ticket;
  ulong * h_tick; void * m_tick;
  int     tick_arm;
  ulong   a_dbase;
};

#define FD_AMD_SLOT_MAX (FD_ED25519_AMD_SLOT_MAX)

struct fd_ed25519_amd {
  int    device;
  ulong  cap;        /* signatures per chunk */
  ulong  blob_cap;   /* message bytes per chunk */
  int    nslot;      /* slots the SoA calls keep in flight: 2 (double buffering), or FD_ED25519_AMD_NSLOT */
  int    mode;       /* FD_ED25519_AMD_MODE_*: mirrored into every slot's `strict` */
  int    gather_copy;/* verify_batch_registered: 0 k_gather reads a chunk's records in the mapped h_pack (default),
                        1 they go to d_pack by one H2D first (FD_ED25519_AMD_GATHER_COPY=1: the A/B of tools/batch_registered_cost.py) */
  int    gather_txn_waves; /* verify_txns_registered: wave cap of a throughput chunk's k_gather_txn, 64 (default), or
                              FD_ED25519_AMD_GATHER_TXN_WAVES in [1, 65536] (the A/B of tools/txns_registered_cost.py) */
  /* asynchronous submissions: slots [0, nslot) taken round robin.  a_cnt in
     flight, the oldest on slot a_head, the next goes to slot a_tail; ticket:
     the last one handed out.  While a_cnt > 0 the synchronous calls refuse
     (they would reuse the slots). */
  ulong  ticket;
  int    a_head, a_tail, a_cnt;
  int    poll_event; /* 0 fd_ed25519_amd_async_poll reads the slot's completion word (default), 1 it asks
                        hipEventQuery and no k_ticket is launched (FD_ED25519_AMD_ASYNC_POLL=event: the A/B of
                        tools/async_cost.py) */
  uint8_t * h_tickbuf; /* the slots' completion words, one allocation, 64 bytes each */
  ulong  salt;         /* the survivor filter's table salt: drawn once at creation from the OS (getrandom; a clock if
                          that fails), mirrored into every slot */
  fd_ed25519_amd_window_t * win;   /* the dedup window the _keep submissions filter against and feed (borrowed; NULL: none) */
  slot_t slot[FD_AMD_SLOT_MAX];
};

/* A dedup window (fd_ed25519_window.cpp; include/fd_ed25519_amd.h, "The
   dedup window").  device < 0: host-only, the state lives in h_ring / h_key /
   h_stamp and fd_ed25519_amd_window_keep runs the rule on it.  Otherwise the
   same four arrays lie in d_state (fd_amd_win_layout( depth )) and only the
   kernels of fd_ed25519_window.h touch them.  since: the items offered since
   the map was last rebuilt (the host's bound on the keys it holds beyond the
   live ones).  seq: the submissions that acted on a device window, whose
   parity says which head word holds the count.  owner: the engine the window is attached to.  pend: the event
   recorded behind the last launch that touched the window (own_ev for
   fd_ed25519_amd_window_keep_dev, a slot's win_done for an engine's
   submission), NULL when nothing is queued. */
struct fd_ed25519_amd_window_s {
  int     device;
  ulong   depth, salt, cap, since, seq;
  ulong * h_ring; ulong * h_key; ulong * h_stamp; ulong h_head;
  uint8_t * d_state;
  struct fd_ed25519_amd * owner;
  hipEvent_t own_ev, pend;
};

#ifdef FD_ED25519_KERNELS_H
/* The launch's view of a device window for a submission of n items, which
   it counts into `since`: a rebuild goes first whenever the items offered
   since the last one, these included, exceed depth.  n > 0 is a submission
   and takes the next head word; n == 0 (import's rebuild) stays on this one.
   done: the event to record behind the window's kernels; it becomes the
   window's pending one, and the one pending now is waited for unless it is
   the same (then the stream orders the two). */
static inline fd_amd_win_dev_t
fd_amd_window_arm( fd_ed25519_amd_window_t * w, ulong n, hipEvent_t done ) {
  fd_amd_win_layout_t L = fd_amd_win_layout( w->depth );
  fd_amd_win_dev_t d;
  d.ring = (uint64_t *)(w->d_state + L.ring); d.head  = (uint64_t *)(w->d_state + L.head);
  d.key  = (uint64_t *)(w->d_state + L.key);  d.stamp = (uint64_t *)(w->d_state + L.stamp);
  d.depth = w->depth; d.salt = w->salt; d.cap = (uint32_t)L.cap;
  d.rebuild = w->since + n > w->depth;
  w->since = d.rebuild ? n : w->since + n;
  d.cur = (uint32_t)( w->seq & 1UL );
  if( n ) w->seq++;
  d.wait = w->pend != done ? w->pend : NULL; d.done = done;
  if( done ) w->pend = done;
  return d;
}
#endif

/* NUMA placement (fd_numa.cpp): bind the calling thread to the device's
   node (CPUs + preferred memory), or prefer it only while allocating. */
int  fd_amd_numa_bind_thread( int device );
int  fd_amd_numa_prefer_begin( int device, int * saved_mode, unsigned long * saved_mask /* 16 words */ );
void fd_amd_numa_prefer_end( int saved_mode, unsigned long const * saved_mask );

static inline bool
fd_amd_mode_ok( int mode ) {
  return mode == FD_ED25519_AMD_MODE_REFERENCE || mode == FD_ED25519_AMD_MODE_STRICT;
}

/* The argument checks of the SoA and the transaction batch calls (the
   multi-device engine makes them once for the whole batch, so either every
   shard runs or none): FD_ED25519_AMD_OK or FD_ED25519_AMD_ERR_INVAL, before
   anything launches, so an error never leaves a chunk in flight and the
   chunk loop always makes progress.  SoA: every message in bounds and small
   enough for one chunk.  Transactions: each in bounds and stageable in one
   chunk (its bytes in blob_max, its signatures in batch_max); sig_base given
   whenever a per-signature output (sig_err, sig_tag) is; desc and desc_off
   both or neither, with room for the sum of fd_txn_amd_desc_bound. */
int fd_amd_soa_args_check( fd_ed25519_amd_t const * e, ulong n, uchar const * pub, uchar const * sig, uint const * msg_off,
                           uint const * msg_sz, uchar const * blob, ulong blob_sz, schar const * err );
int fd_amd_txn_args_check( fd_ed25519_amd_t const * e, ulong txn_cnt, uchar const * payload, uint const * txn_off,
                           uint const * txn_sz, ulong payload_sz, schar const * txn_err, uint const * sig_base,
                           schar const * sig_err, ulong const * sig_tag, ulong const * desc_off = NULL,
                           uchar const * desc = NULL, ulong desc_cap = 0UL );

/* signature slots reserved for a payload (fd_txn_parse.c:79-82 rule) */
ulong fd_amd_txn_slots1( uchar const * p, ulong sz );

#endif
