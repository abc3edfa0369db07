/* firedancer_amd/csrc/fd_ed25519_kernels.h -- internal interface between
   the host engine (fd_ed25519_engine.cpp) and the HIP kernels. */
#ifndef FD_ED25519_KERNELS_H
#define FD_ED25519_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

typedef struct {
  size_t N;      /* n rounded up to 64 */
  size_t dig, evn, top, A, R, Ai, st, tag, ds, init, ctr;   /* byte offsets of the workspace planes */
  size_t total;  /* footprint in bytes */
} ws_layout_t;

ws_layout_t fd_amd_ws_layout( size_t n );

/* Enqueue k_prep -> k_decomp -> k_dsm on `stream`; when ev != NULL record
   ev[0..3] before/between/after the three kernels.  d_skip (NULL = none):
   per-signature int8, nonzero = do not verify, the verdict is that value
   (transaction slots whose payload failed to parse).  0 on success. */
int fd_amd_launch_verify( uint32_t n, uint8_t const * d_pub, uint8_t const * d_sig, uint32_t const * d_off,
                          uint32_t const * d_sz, uint8_t const * d_blob, int8_t * d_err, void * d_ws,
                          hipStream_t stream, int want_stats, hipEvent_t const * ev /* 4 or NULL */,
                          int8_t const * d_skip = NULL, int dsm_mode = 0, int8_t * d_out = NULL, int strict = 0 );
/* d_out (NULL = none): on the latency path (fd_amd_uses_latency_path) the
   last kernel also writes every verdict to d_out, e.g. mapped host memory,
   so the caller needs no copy kernel; the throughput path ignores it.
   strict (FD_ED25519_AMD_MODE_STRICT): also enqueue k_strict after the DSM
   stage (after k_fin on the pooled path, before ev[3]); it turns d_err into
   the strict verdicts and is then the kernel that writes d_out. */
/* Verdict byte that marks every signature of a launch whose k_dsmp hang
   guard tripped (never a reference code): the host calls turn it into
   FD_ED25519_AMD_ERR_DEVICE. */
#define FD_AMD_VERDICT_DEVICE (-128)
/* dsm_mode: 0 = by batch size (fd_ed25519_amd_set_latency_batch_max,
   fd_ed25519_amd_set_small_batch_max), 1 = the throughput path (k_prep,
   k_decomp, k_dsm), 2 = k_front + k_dsm4, 3 = k_front + k_dsm8, 4 = the
   throughput path with the pooled DSM (k_ai, k_dsmp, k_fin). */

/* Transaction front end (fd_txn_kernels.hip).
   k_txn_parse: one lane per transaction t = d_payload[d_toff[t] .. +d_tsz[t]).
     d_fp[t] = fd_txn_parse return value; d_out (optional) + t*out_stride gets
     the fd_txn_t descriptor: the header, and every instruction and
     lookup-table record that ends within out_stride (all of them when
     d_fp[t] <= out_stride).  When d_tbase != NULL it also lays out the
     transaction's signatures for the verify kernels at slots
     [d_tbase[t], d_tbase[t+1]): pub/sig copied from the payload, msg_off/msg_sz
     pointing at the shared message inside d_payload, skip = 0; a payload that
     fails to parse marks its slots skip = FD_TXN_AMD_ERR_PARSE.
   k_txn_reduce: d_terr[t] = parse failure code, or the first nonzero
     verdict among the transaction's slots, or 0. */
int fd_amd_launch_txn_parse( uint32_t txn_cnt, uint8_t const * d_payload, uint32_t const * d_toff,
                             uint32_t const * d_tsz, uint32_t * d_fp, uint8_t * d_out, size_t out_stride,
                             uint32_t const * d_tbase, uint8_t * d_pub, uint8_t * d_sig, uint32_t * d_off,
                             uint32_t * d_sz, int8_t * d_skip, hipStream_t stream );
int fd_amd_launch_txn_reduce( uint32_t txn_cnt, uint32_t const * d_fp, uint32_t const * d_tbase,
                              int8_t const * d_err, int8_t * d_terr, hipStream_t stream );

/* Compute budget (fd_txn_budget.h: k_txn_budget), after a k_txn_parse that
   left d_fp: d_budget[t], a 24-byte fd_txn_amd_budget_t, for every
   t < txn_cnt (device or mapped host memory, 8-aligned), and nothing else. */
int fd_amd_launch_txn_budget( uint32_t txn_cnt, uint8_t const * d_payload, uint32_t const * d_toff, uint32_t const * d_tsz,
                              uint32_t const * d_fp, void * d_budget, hipStream_t stream );

/* Packed descriptors (fd_txn_kernels.hip), after a k_txn_parse that left
   d_fp: d_desc_off[0 .. txn_cnt] = the 64-bit exclusive prefix sum of d_fp
   (d_desc_off[txn_cnt] the total) and, for every t with d_fp[t] != 0 and
   d_desc_off[t+1] <= desc_cap, the descriptor at d_desc + d_desc_off[t]
   (d_desc 2-aligned); no byte at or beyond d_desc + desc_cap is written.
   d_bsum: scratch, one u64 per 64 transactions.  Three kernels ordered by
   the stream (txn_cnt == 0: the one that writes d_desc_off[0]); no workgroup
   waits for another.
   fd_amd_launch_desc_out: d_desc_off[0 .. txn_cnt] and the first
   min( d_desc_off[txn_cnt], cap ) packed bytes, rounded up to 16, to mapped
   host memory by a kernel that reads the total on the device; all four
   buffers are 16-aligned and the byte buffers hold round_up( cap, 16 )
   bytes.  bound: what
   the host knows the total cannot exceed (sizes the grid only). */
int fd_amd_launch_txn_pack( uint32_t txn_cnt, uint8_t const * d_payload, uint32_t const * d_toff, uint32_t const * d_tsz,
                            uint32_t const * d_fp, uint64_t * d_bsum, uint64_t * d_desc_off, uint8_t * d_desc,
                            uint64_t desc_cap, hipStream_t stream );
/* The scan's first two kernels alone, over any plane of n u32 values (every
   64 of them summing below 2^32): d_bsum[b] = the sum of the 64-blocks before
   block b, *d_total = the sum of all; n == 0 writes *d_total = 0 only. */
int fd_amd_launch_scan64( uint32_t n, uint32_t const * d_val, uint64_t * d_bsum, uint64_t * d_total, hipStream_t stream );
int fd_amd_launch_bscan64( uint32_t nblk, uint64_t * d_bsum, uint64_t * d_total, hipStream_t stream );
int fd_amd_launch_desc_out( void * d_dst_mapped, uint8_t const * d_desc, void * d_off_mapped, uint64_t const * d_desc_off,
                            uint32_t txn_cnt, uint64_t cap, uint64_t bound, hipStream_t stream );

/* GPU keygen + sign (fd_ed25519_sign.hip): prv[n][32] seeds, messages
   blob[off[i] .. +sz[i]) -> pub[n][32], sig[n][64].  0 on success. */
int fd_amd_launch_sign( uint32_t n, uint8_t const * d_prv, uint32_t const * d_off, uint32_t const * d_sz,
                        uint8_t const * d_blob, uint8_t * d_pub, uint8_t * d_sig, hipStream_t stream );

/* Streaming tile, persistent consumer (k_tile_persist).  One launch per
   tile run; its waves take chunk descriptors the tile's host thread
   publishes in mapped host memory and verify them, so the GPU never drains
   between hand-offs and the tile needs one stream (one hardware queue).

   ring entry (host -> GPU): the frag's chunk in the source region, its
   output frame's chunk (zero-copy: the GPU writes the verified bytes
   there), its size, and (TXN framing) its signature slots
   (fd_amd_txn_slots1).  Entry of ring index j at ent[j & mask]. */
typedef struct { uint32_t src_chunk, out_chunk, sz, slots; } fd_amd_tile_ent_t;
/* chunk descriptor (host -> GPU): ring entries [first, first + count),
   count <= 64 | FD_AMD_TILE_LAT (8 lanes per signature) or FD_AMD_TILE_QUAD
   (4 lanes per signature); the entries' signature slots total <= 64 (<= 8
   in a latency chunk, <= 16 in a quad chunk) */
typedef struct { uint64_t first; uint32_t count; uint32_t pad; } fd_amd_tile_desc_t;   /* pad: pair sub | seq << 1 */
#define FD_AMD_TILE_LAT  (0x80000000u)
#define FD_AMD_TILE_QUAD (0x40000000u)
/* a quad PAIR (PUB_SIG_MSG): two descriptors over the same 17..32 entries,
   pad = sub | pair_seq << 1.  Sub 0 hashes and decompresses all of them
   into pair workspace pair_seq & pair_mask, raises its flag, and verifies
   entries 0..15; sub 1 waits for the flag and verifies entries 16.. -- one
   front pass (all lanes busy) serves two quad chunks */
#define FD_AMD_TILE_PAIR (0x20000000u)
#define FD_AMD_TILE_COUNT(c) ((c) & 0x1fffffffu)
/* result of ring index j (GPU -> host), two arrays of R words: tag[j & mask]
   and word[j & mask] = (j + 1) << 8 | (uint8_t)verdict, the word stored
   after the tag and after the frag's output bytes (system-scope release),
   so a host that sees word's index also sees the rest.  Arrays, not
   {tag, word} records: a chunk's 64 lanes then store 512 contiguous bytes
   per instruction (whole lines) -- interleaved 8-B stores into mapped host
   memory held the L2 so long that every wave of the GPU slowed ~5x
   (tools/tile_synth.py, profiles/r03_tile_persist_ab.txt). */
/* control words in mapped host memory, each on its own 64-B line: the
   first three are written by the host, the last by the GPU's scout */
typedef struct {
  uint64_t head;  uint64_t pad0[7];   /* chunk descriptors [.., head) are published to the GPU */
  uint64_t beat;  uint64_t pad1[7];   /* host heartbeat: the kernel's watchdog */
  uint32_t stop;  uint32_t kerr;  uint64_t pad2[7];   /* stop: exit once drained; kerr: set by the kernel on a watchdog exit */
  uint64_t gclock;                    /* scout: its s_memrealtime (100 MHz), every ~10 us; nonzero = the kernel started */
  uint64_t gdone;                     /* scout: chunks the waves finished (mirror of dctl->done) */
  uint64_t pad3[6];
} fd_amd_tile_hctl_t;
/* device control block (zeroed by the host before each launch) */
#define FD_AMD_TILE_MIRRORS (8)
typedef struct { uint64_t w; uint64_t pad[7]; } fd_amd_tile_mirror_t;
typedef struct {
  uint64_t             ticket;  uint64_t pad0[7];   /* next chunk ticket (one atomic add per chunk) */
  fd_amd_tile_mirror_t mw[FD_AMD_TILE_MIRRORS];     /* per XCD: descriptor head | heartbeat << 48 | err << 62 | stop << 63 */
  uint64_t             done;    uint64_t pad1[7];   /* chunks finished (one atomic add per chunk; the scout mirrors it) */
  uint64_t             stat[6];                     /* chunks in latency mode, in throughput mode; frags in each; quad chunks, their frags */
  uint64_t             prof[8];                     /* diagnostics build (FD_AMD_DIAG, args.prof): summed ticks gather, decomp, DSM, results, wait, fence, prep */
} fd_amd_tile_dctl_t;
typedef struct {
  fd_amd_tile_hctl_t *       hctl;     /* device address of the mapped control words */
  fd_amd_tile_ent_t const *  ent;      /* device address of the mapped ring */
  fd_amd_tile_desc_t const * desc;     /* device address of the mapped chunk descriptors (same size as the ring) */
  uint64_t *                 res_tag;  /* device address of the mapped results: tags */
  uint64_t *                 res_word; /*   and verdict words */
  uint64_t *                 res_time; /*   and (NULL = none) per frag: claim | done << 32, low 32 bits of the
                                            s_memrealtime ticks when its wave took the chunk and stored its results */
  uint64_t                   mask;     /* ring size - 1 (power of 2) */
  uint8_t const *            src;      /* frag source region (mapped): input dcache (zero-copy) or the output frames */
  uint8_t *                  out;      /* output frames (mapped) to fill, or NULL (copy mode: the host filled them) */
  fd_amd_tile_dctl_t *       dctl;
  uint8_t *                  scratch;  /* per-wave scratch, fd_amd_tile_scratch_stride() bytes apart */
  uint64_t                   watchdog; /* s_memrealtime ticks (100 MHz) without a host heartbeat before the kernel gives up */
  uint32_t                   prof;     /* diagnostics build only: sum per-phase time stamps into dctl->prof */
  uint32_t                   txn;      /* TXN framing: entries are wire transactions, results per transaction */
  uint8_t *                  pair_ws;  /* quad pairs: pair_mask + 1 workspaces, fd_amd_tile_scratch_stride() apart */
  uint32_t *                 pair_flag;/*   and their flags (pair_seq + 1 once a pair's front is done) */
  uint32_t                   pair_mask;
  uint32_t                   pad_;
} fd_amd_tile_args_t;
size_t fd_amd_tile_scratch_stride( void );
/* waves: grid size (wave 0 is the scout that mirrors the host words);
   strict: 0 launches k_tile_persist (the reference's verdicts), nonzero
   k_tile_persist_strict (the strict overlay inside every chunk) */
int fd_amd_launch_tile_persist( fd_amd_tile_args_t const * a, uint32_t waves, hipStream_t stream, int strict );   /* 0, -1 (waves), or a hipError_t */

#ifdef FD_AMD_DIAG
/* diagnostics build: the chunk pipeline alone, every argument in device memory */
int fd_amd_launch_tile_synth( fd_amd_tile_args_t const * a, uint32_t waves, uint32_t iters, int eight, hipStream_t stream );
#endif

/* Dense slide digits of the last call on workspace d_ws (debug): u16
   [n][256] (low byte h digit, high byte s digit) rebuilt from the event
   lists k_prep writes. */
int fd_amd_launch_digits_dense( uint32_t n, void const * d_ws, uint16_t * d_dig, hipStream_t stream );

/* 1 when a batch of n takes the latency kernels (k_front + k_dsm8/k_dsm4). */
int fd_amd_uses_latency_path( uint32_t n, int dsm_mode );

/* The DSM kernel fd_amd_launch_verify runs for a batch of n: 1 k_dsm,
   2 k_dsm4, 3 k_dsm8, 4 k_dsmp (FD_ED25519_AMD_DSM_*). */
int fd_amd_dsm_kind( uint32_t n, int dsm_mode );

/* R' of the last call on workspace d_ws (debug): int32 [30][n], the X | Y | Z
   limbs DSM kernel `kind` parked per signature (0 = the kernel the size rule
   gives a batch of n now); defined only where the DSM ran. */
int fd_amd_launch_rprime( uint32_t n, void const * d_ws, int kind, int32_t * d_xyz, hipStream_t stream );

/* d_off[i] -= lo for every nonempty message (0 for empty ones). */
int fd_amd_launch_rebase_off( uint32_t n, uint32_t * d_off, uint32_t const * d_sz, uint32_t lo, hipStream_t stream );

/* k_gather (fd_ed25519_gather.h): n records -> the verify planes.  A record
   is one signature of a pointer-array chunk: the DEVICE addresses of its
   public key (32 B), signature (64 B) and message (sz B; unused when sz is
   0), any byte alignment, in host memory the GPU can read; dst: a multiple
   of 16, the message's offset in d_blob, which owns
   [dst, dst + round_up( sz, 16 )) there.  d_rec: 32-aligned device or mapped
   host memory.  Writes d_pub[32 i], d_sig[64 i], d_off[i] = dst,
   d_sz[i] = sz, d_blob[dst ..]. */
typedef struct { uint64_t pub, sig, msg; uint32_t sz, dst; } fd_amd_gather_rec_t;
int fd_amd_launch_gather( uint32_t n, fd_amd_gather_rec_t const * d_rec, uint8_t * d_pub, uint8_t * d_sig,
                          uint32_t * d_off, uint32_t * d_sz, uint8_t * d_blob, uint32_t waves, hipStream_t stream );

/* k_gather_txn (fd_ed25519_gather.h): n records -> the transaction planes.
   A record is one payload of a pointer-array transaction chunk: src, the
   DEVICE address of its sz <= FD_TXN_AMD_MTU bytes (unused when sz is 0),
   any byte alignment, in host memory the GPU can read; dst: a multiple of
   16, the payload's offset in d_blob, which owns
   [dst, dst + round_up( sz, 16 )) there; tbase: its first signature slot.
   d_rec: 32-aligned device or mapped host memory.  Writes d_blob[dst ..],
   d_toff[t] = dst, d_tsz[t] = sz, d_tbase[t] = tbase and
   d_tbase[n] = slot_cnt.  At most `waves` waves (0: no cap). */
typedef struct { uint64_t src; uint32_t sz, dst, tbase, pad[3]; } fd_amd_gather_txn_rec_t;
int fd_amd_launch_gather_txn( uint32_t n, fd_amd_gather_txn_rec_t const * d_rec, uint8_t * d_blob, uint32_t * d_toff,
                              uint32_t * d_tsz, uint32_t * d_tbase, uint32_t slot_cnt, uint32_t waves, hipStream_t stream );

/* Frag submissions (fd_ed25519_frags.h; include/fd_tango_amd.h, "Frag
   submissions").  The two statuses a line can give an item, restated from
   the public header (fd_ed25519_engine.cpp asserts the equality).
   fd_amd_launch_frag_list: items [0, n) of the submission ( seq0, n ) over
   d_mcache (depth lines, a power of two; device address, 32-aligned) and the
   data region [d_chunk0, d_chunk0 + data_sz) -> d_rec[0, n), the records
   k_gather consumes with dst = i * round_up( frag_max - 96, 16 ), and
   d_status[0, n) (both device memory; d_rec 32-aligned).  d_idle: 96 zero
   bytes of device memory, 16-aligned.  n * round_up( frag_max - 96, 16 )
   < 2^32.
   fd_amd_launch_frag_check: the recheck of every item whose status is 0.
   fd_amd_launch_frag_verdict: the statuses over the n verdicts d_err (and
   m_err, the mapped copy, when not NULL) and 0 over their tags in the tag
   plane of d_ws, the workspace of a verify launch of n signatures; d_mcache
   != NULL: the recheck first. */
#define FD_AMD_VERDICT_FRAG_SEQ (-5)
#define FD_AMD_VERDICT_FRAG_BAD (-6)
int fd_amd_launch_frag_list( uint32_t n, void const * d_mcache, uint64_t depth, uint64_t seq0, uint64_t d_chunk0,
                             uint64_t data_sz, uint32_t frag_max, uint64_t d_idle, fd_amd_gather_rec_t * d_rec,
                             int8_t * d_status, hipStream_t stream );
int fd_amd_launch_frag_check( uint32_t n, void const * d_mcache, uint64_t depth, uint64_t seq0, int8_t * d_status,
                              hipStream_t stream );
int fd_amd_launch_frag_verdict( uint32_t n, int8_t * d_status, void const * d_mcache, uint64_t depth, uint64_t seq0,
                                int8_t * d_err, int8_t * m_err, void * d_ws, hipStream_t stream );

/* n bytes device -> mapped host memory by a kernel (no DMA engine). */
int fd_amd_launch_copy_out( void * d_dst_mapped, void const * d_src, size_t n, hipStream_t stream );

/* Dedup tags (k_tag_out): the n tags k_prep / k_front left in the tag plane
   of workspace d_ws (the workspace of a verify launch of n signatures) ->
   d_dst, u64 [n], 8-aligned device or mapped host memory.  Gather form:
   d_dst[t] = the tag at slot d_tbase[t] for each of txn_cnt transactions, 0
   for one without a slot; d_ws is the workspace of the verify launch over
   d_tbase[txn_cnt] slots. */
int fd_amd_launch_tag_out( void * d_dst, void const * d_ws, size_t n, hipStream_t stream );
int fd_amd_launch_tag_gather( void * d_dst, void const * d_ws, uint32_t txn_cnt, uint32_t const * d_tbase, hipStream_t stream );

/* Survivors (fd_ed25519_keep.h): d_keep[0 .. *d_keep_cnt) = the ascending
   indices i < n with d_err[i] == 0 that are the first passing item of their
   tag d_tag[i] (tag 0: never a duplicate), *d_keep_cnt their number.  d_tag:
   8-aligned device memory; d_keep (4-aligned, n entries) and d_keep_cnt
   (8-aligned): device or mapped host memory.  d_scratch: fd_amd_keep_layout(
   n ).total bytes of device memory, 256-aligned, contents irrelevant.  Writes
   d_scratch[0, total), d_keep[0, count) and *d_keep_cnt; n == 0 writes
   *d_keep_cnt = 0 only.  d_fp / d_fpk (both or neither): also d_fpk[i] =
   d_fp[i] for a survivor, 0 for every other item.  salt: see the header; no
   output depends on it.  n <= FD_AMD_KEEP_MAX. */
#define FD_AMD_KEEP_MAX (1u << 30)
typedef struct {
  size_t cap;                      /* slots of the table: a power of two >= max( 2 n, 64 ) */
  size_t key, idx, flag, bsum;     /* byte offsets: u64 [cap], u32 [cap], u32 [n], u64 [ceil( n/64 )] */
  size_t total;                    /* footprint in bytes */
} fd_amd_keep_layout_t;
fd_amd_keep_layout_t fd_amd_keep_layout( size_t n );
int fd_amd_launch_keep( uint32_t n, int8_t const * d_err, uint64_t const * d_tag, uint32_t const * d_fp, uint32_t * d_fpk,
                        uint32_t * d_keep, uint64_t * d_keep_cnt, void * d_scratch, uint64_t salt, hipStream_t stream );

/* The dedup window (fd_ed25519_window.h): the survivors of a submission
   filtered against the last `depth` tags earlier submissions published, which
   are then joined by this one's.  fd_amd_win_dev_t: where a window's state
   lies on the device (fd_amd_win_layout( depth ): ring u64 [depth], head u64
   [2], key and stamp u64 [cap], cap a power of two >= max( 4 depth, 256 )),
   its salt, which head word this launch reads (cur: it leaves the new count
   in the other), whether the host wants the map rebuilt ahead of this launch,
   the event to wait for ahead of the window's kernels and the one to record
   behind them (NULL: none).
   fd_amd_launch_keep_win is fd_amd_launch_keep with a window (w == NULL: that
   call exactly): n <= w->depth, and d_scratch holds fd_amd_win_scratch( n )
   .total bytes -- the keep layout first, then flag2 u32 [n] and bsum2 u64
   [ceil( n/64 )].  n == 0 touches no window.  Launches on
   one window must be ordered by the caller (one stream, or events).
   fd_amd_launch_win_rebuild: the rebuild alone (after an import wrote ring
   and head[cur]). */
typedef struct {
  uint64_t * ring; uint64_t * head; uint64_t * key; uint64_t * stamp;
  uint64_t   depth, salt;
  uint32_t   cap, cur;
  int        rebuild;
  hipEvent_t wait, done;
} fd_amd_win_dev_t;
typedef struct { size_t cap, ring, head, key, stamp, total; } fd_amd_win_layout_t;
typedef struct { size_t flag2, bsum2, total; } fd_amd_win_scratch_t;
fd_amd_win_layout_t  fd_amd_win_layout( size_t depth );
fd_amd_win_scratch_t fd_amd_win_scratch( size_t n );
int fd_amd_launch_win_rebuild( fd_amd_win_dev_t const * w, hipStream_t stream );
int fd_amd_launch_keep_win( uint32_t n, int8_t const * d_err, uint64_t const * d_tag, uint32_t const * d_fp, uint32_t * d_fpk,
                            uint32_t * d_keep, uint64_t * d_keep_cnt, void * d_scratch, uint64_t salt,
                            fd_amd_win_dev_t const * w, hipStream_t stream );

/* Output frames (fd_ed25519_emit.h): for j < cnt = min( *d_keep_cnt, n ) the
   frame of item d_keep[j] at d_out + d_emit_off[j], d_emit_sz[j] bytes; an
   item >= n (or one too large for a frame) has size 0.  d_emit_off[0 .. cnt]
   and d_emit_sz[0 .. cnt) are always complete; frame j is stored only if
   d_emit_off[j+1] <= out_cap.  d_out: 64-aligned, device or mapped host
   memory; d_keep / d_keep_cnt / d_emit_off (8-aligned) / d_emit_sz: device or
   mapped host memory; d_scratch: fd_amd_emit_layout( n ).total bytes of
   device memory, 256-aligned, contents irrelevant.  The store kernel runs at
   most `waves` waves (0: one per block of frames).  Signature form: the five
   verify planes.  Transaction form: the payload planes and the packed
   descriptors (d_desc_off: n + 1 entries).  n <= FD_AMD_KEEP_MAX. */
typedef struct { size_t idx, esz, units, off, bsum, word, total; } fd_amd_emit_layout_t;
fd_amd_emit_layout_t fd_amd_emit_layout( size_t n );
int fd_amd_launch_emit_sig( uint32_t n, uint8_t const * d_pub, uint8_t const * d_sig, uint32_t const * d_msg_off,
                            uint32_t const * d_msg_sz, uint8_t const * d_blob, uint32_t const * d_keep,
                            uint64_t const * d_keep_cnt, void * d_out, uint64_t out_cap, uint64_t * d_emit_off,
                            uint32_t * d_emit_sz, void * d_scratch, uint32_t waves, hipStream_t stream );
int fd_amd_launch_emit_txn( uint32_t txn_cnt, uint8_t const * d_payload, uint32_t const * d_txn_off, uint32_t const * d_txn_sz,
                            uint64_t const * d_desc_off, uint8_t const * d_desc, uint32_t const * d_keep,
                            uint64_t const * d_keep_cnt, void * d_out, uint64_t out_cap, uint64_t * d_emit_off,
                            uint32_t * d_emit_sz, void * d_scratch, uint32_t waves, hipStream_t stream );

/* k_ticket (fd_ed25519_async.hip): one lane stores `ticket` to the 8-aligned
   word at d_word (mapped host memory) with a system-scope release store, behind
   whatever the stream holds. */
int fd_amd_launch_ticket( void * d_word, uint64_t ticket, hipStream_t stream );

#endif
