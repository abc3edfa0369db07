#ifndef HEADER_fd_ed25519_amd_h
#define HEADER_fd_ed25519_amd_h

/* MI355X ed25519 batch-verification engine -- the C-ABI drop-in boundary.
 *
 * Library: firedancer_amd/libfd_ed25519_amd.so (hipcc, gfx950).
 *
 * Part 1 reproduces the reference's public API for the verify path
 * (lijunwangs/firedancer src/ballet/ed25519/fd_ed25519.h), same names,
 * same argument meaning, same return codes, so an existing caller (the
 * verify tile, the Rust re-export ffi/rust/firedancer-sys/src/ballet/
 * ed25519.rs:1-10) relinks against this library unchanged.  Verdicts are
 * bit-exact with the reference's DEFAULT x86_64 (AVX) build, including its
 * documented non-strict behaviours.
 *
 * Part 2 is new: batch entry points (the reference only verifies one
 * signature per call).  Every verdict they return equals what Part 1's
 * fd_ed25519_verify returns for the same inputs -- by default.  An engine
 * may opt in to strict RFC 8032 verdicts instead (fd_ed25519_amd_set_mode,
 * FD_ED25519_AMD_MODE_STRICT below).
 *
 * All verify work runs on the GPU.  There is no CPU fallback: without a
 * usable HIP device every verify entry point returns FD_ED25519_AMD_ERR_DEVICE
 * (batch API) or aborts with a message (drop-in API, which has no error code
 * for "no device").
 */

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef unsigned char uchar;
typedef unsigned long ulong;
typedef unsigned int  uint;
typedef signed char   schar;

/* ===== Part 1: reference API (src/ballet/ed25519/fd_ed25519.h) ===== */

/* fd_ed25519.h:11-14 */
#define FD_ED25519_SUCCESS    ( 0) /* Operation was succesful */
#define FD_ED25519_ERR_SIG    (-1) /* signature obviously invalid (s check) */
#define FD_ED25519_ERR_PUBKEY (-2) /* public key (or R) failed to decompress */
#define FD_ED25519_ERR_MSG    (-3) /* message didn't match the signature */

/* fd_ed25519.h:17-20 */
#define FD_ED25519_SIG_SZ (64UL)
typedef uchar fd_ed25519_sig_t[ FD_ED25519_SIG_SZ ];

/* The reference passes a caller-owned SHA-512 calculator as scratch
   (fd_ed25519.h:81-95; src/ballet/sha512/fd_sha512.h:15-16,56-77: 256 B,
   128-aligned).  This library hashes on the GPU and only takes the
   reference's write interest in it; it never dereferences it.  A caller
   that already includes the reference's fd_sha512.h keeps its definition. */
#ifndef FD_SHA512_ALIGN
#define FD_SHA512_ALIGN     (128UL)
#define FD_SHA512_FOOTPRINT (256UL)
typedef struct fd_sha512_private fd_sha512_t;
#endif

/* fd_ed25519_verify -- replaces fd_ed25519.h:96-101 (impl
   fd_ed25519_user.c:345-431).  Returns FD_ED25519_SUCCESS or an
   FD_ED25519_ERR_* code, bit-exact with the reference.  Reentrant; runs as
   a batch of one on the calling thread's own engine, on the thread's
   device (fd_ed25519_amd_dropin_set_device below).  msg==NULL fine when
   sz==0. */
int
fd_ed25519_verify( void const *  msg,
                   ulong         sz,
                   void const *  sig,
                   void const *  public_key,
                   fd_sha512_t * sha );

/* Device routing of the drop-in call.  The reference runs N verify tiles
   as threads of one process (src/app/frank/fd_frank_main.c:118-143), each
   calling fd_ed25519_verify (fd_frank_verify_synth_load.c:380), so the
   device is chosen per calling thread:
   - fd_ed25519_amd_dropin_set_device( d ) (d >= 0) from the thread (e.g. at
     its tile's boot) pins the thread's calls to HIP device d; its next call
     moves its engine there.  FD_ED25519_AMD_DROPIN_AUTO returns the thread
     to the default.  0, ERR_INVAL (d < -1 or not a device) or ERR_DEVICE
     (no HIP).
   - default (picked once, at the thread's first call):
     FD_ED25519_AMD_DEVICE when set; else round robin over the GPUs on the
     NUMA node of the CPU the thread runs on (a tile pinned to a core gets a
     GPU of its own socket), over all GPUs when none is local: the rule of
     fd_ed25519_amd_dropin_pick, with ordinal = the threads of that node that
     took a default before it.
   fd_ed25519_amd_dropin_device: the device of the calling thread's engine
   (-1 before its first call).  fd_ed25519_amd_dropin_pick (pure): of
   dev_cnt devices on NUMA nodes dev_node[] (-1 unknown), the device for
   the ordinal-th thread on node cpu_node (-1 unknown). */
#define FD_ED25519_AMD_DROPIN_AUTO    (-1)
#define FD_ED25519_AMD_DROPIN_DEV_MAX (64)
int
fd_ed25519_amd_dropin_set_device( int device );

int
fd_ed25519_amd_dropin_device( void );

int
fd_ed25519_amd_dropin_pick( int const * dev_node, int dev_cnt, int cpu_node, ulong ordinal );

/* fd_ed25519_strerror -- replaces fd_ed25519.h:108-109 (impl
   fd_ed25519_user.c:433-443): same strings. */
char const *
fd_ed25519_strerror( int err );

/* fd_ed25519_public_from_private / fd_ed25519_sign -- replace
   fd_ed25519.h:40-78 (impl fd_ed25519_user.c:279-343).  Host-side (not
   the verify hot path); deterministic RFC 8032 signing, so the bytes equal
   the reference's. */
void *
fd_ed25519_public_from_private( void *        public_key,
                                void const *  private_key,
                                fd_sha512_t * sha );

void *
fd_ed25519_sign( void *        sig,
                 void const *  msg,
                 ulong         sz,
                 void const *  public_key,
                 void const *  private_key,
                 fd_sha512_t * sha );

/* ===== Part 2: batch engine (new) ===== */

#define FD_ED25519_AMD_OK          ( 0)
#define FD_ED25519_AMD_ERR_INVAL   (-10) /* bad argument (NULL, n too large, a message larger than the engine's blob_max) */
#define FD_ED25519_AMD_ERR_DEVICE  (-11) /* HIP error / no device */
#define FD_ED25519_AMD_ERR_BUSY    (-12) /* a submit call: every slot of the engine carries a submission */
#define FD_ED25519_AMD_ASYNC_NONE  ( 1)  /* async_poll / async_wait: nothing to deliver (not an error) */
#define FD_ED25519_AMD_SLOT_MAX    (16)  /* most slots (chunks in flight) an engine can have */

/* Solana MTU: the message size the staging is dimensioned
   for.  Longer messages verify too, as long as each fits the engine's
   blob_max (the drop-in fd_ed25519_verify grows its engine as needed). */
#define FD_ED25519_AMD_MSG_MAX     (1232UL)

typedef struct fd_ed25519_amd fd_ed25519_amd_t;

/* Create an engine bound to HIP device `device`, able to verify up to
   batch_max signatures whose messages total at most blob_max bytes per
   call (larger calls are split internally).  Owns its HIP stream, device
   buffers and pinned, double-buffered host staging.  NULL on failure.
   One engine per host thread; engines on different devices run
   independently (multi-GPU = one engine per device).  Chunks in flight:
   2, or FD_ED25519_AMD_NSLOT (2..6) from the environment. */
fd_ed25519_amd_t *
fd_ed25519_amd_new( int device, ulong batch_max, ulong blob_max );

/* fd_ed25519_amd_new with the slot count as an argument: slots in
   [2, FD_ED25519_AMD_SLOT_MAX], NULL otherwise (checked before anything
   touches a device).  fd_ed25519_amd_new is this call with 2, or
   FD_ED25519_AMD_NSLOT.  The slot count is the engine's depth for the
   asynchronous calls below. */
fd_ed25519_amd_t *
fd_ed25519_amd_new_slots( int device, ulong batch_max, ulong blob_max, ulong slots );

void
fd_ed25519_amd_delete( fd_ed25519_amd_t * eng );

/* Verdict mode, per engine (no process-wide state; engines are
   independent).  An engine starts in FD_ED25519_AMD_MODE_REFERENCE: every
   verdict equals the reference's default build bit for bit, including
   three behaviours a network-facing caller does not want (DESIGN.md,
   "Reproduced, not fixed"): s values with s[31]==0x10 and a nonzero byte in
   s[16..30] are ACCEPTED without looking at A, R or M; small-order and
   non-canonical points are accepted (A = R = identity, s = 0 verifies any
   message); and about 1.6e-6 of valid signatures are rejected with -3.

   FD_ED25519_AMD_MODE_STRICT returns the strict RFC 8032 verdict instead,
   decided in this order for (msg, sig, pub):
     1. s = LE(sig[32:64]) >= L                        -> FD_ED25519_ERR_SIG
     2. A = pub or R = sig[0:32]: y = LE(bytes) mod 2^255 >= p, or not on
        the curve, or x = 0 with the sign bit set, or one of the 8 torsion
        points ([8]P = identity)                       -> FD_ED25519_ERR_PUBKEY
     3. [s]B - [h]A != R as points, h = SHA-512(R||A||M) mod L
                                                       -> FD_ED25519_ERR_MSG
     4. otherwise                                      -> FD_ED25519_SUCCESS
   A reference -1 or -2 stays -1 / -2.  The mode applies to every entry
   point of the engine (verify_batch, verify_soa, verify_soa_registered,
   verify_txns and the multi-engine forms); the workspace footprint is the
   same.  It costs one more small kernel per batch (measured in
   profiles/strict_cost.json).  The streaming verify tile has a verdict
   mode of its own with the same rule (fd_verify_amd_tile_set_verdict_mode,
   include/fd_tango_amd.h; cost in profiles/tile_strict_cost.json).  Not
   covered: the drop-in fd_ed25519_verify, which is the reference's API and
   keeps the reference's verdicts.

   fd_ed25519_amd_set_mode: FD_ED25519_AMD_OK, or FD_ED25519_AMD_ERR_INVAL
   for any other mode (nothing touches a device).  Call it between batches.
   fd_ed25519_amd_mode: the engine's mode. */
#define FD_ED25519_AMD_MODE_REFERENCE (0)   /* default: the reference's verdicts, bit for bit */
#define FD_ED25519_AMD_MODE_STRICT    (1)   /* the rule above */
int
fd_ed25519_amd_set_mode( fd_ed25519_amd_t * eng, int mode );

int
fd_ed25519_amd_mode( fd_ed25519_amd_t const * eng );

/* Pointer-array batch (the shape of n independent fd_ed25519_verify
   calls): msg[i] (sz[i] bytes), sig[i] (64 B), pub[i] (32 B) -> err[i]
   in {0,-1,-2,-3}.  Host memory, caller-owned, read-only except err.
   Returns FD_ED25519_AMD_OK or a negative FD_ED25519_AMD_ERR_*. */
int
fd_ed25519_amd_verify_batch( fd_ed25519_amd_t *   eng,
                             ulong                n,
                             void const * const * msg,
                             ulong const *        sz,
                             void const * const * sig,
                             void const * const * pub,
                             schar *              err );

/* SoA host batch: pub[n][32], sig[n][64], message i is
   blob[msg_off[i] .. msg_off[i]+msg_sz[i]).  Staged through pinned memory
   (double-buffered, copies overlap the previous chunk's kernels). */
int
fd_ed25519_amd_verify_soa( fd_ed25519_amd_t * eng,
                           ulong              n,
                           uchar const *      pub,
                           uchar const *      sig,
                           uint const *       msg_off,
                           uint const *       msg_sz,
                           uchar const *      blob,
                           ulong              blob_sz,
                           schar *            err );

/* Zero-copy host batch.  fd_ed25519_amd_host_register pins [base,
   base+sz) of caller memory once (hipHostRegister, portable to every
   device; FD_ED25519_AMD_ERR_DEVICE if the runtime refuses).  When pub,
   sig, msg_off, msg_sz and blob all lie in registered memory,
   fd_ed25519_amd_verify_soa_registered moves each chunk's planes and its
   message window from the caller's memory to the device by DMA, with no
   host-side copy (fd_ed25519_amd_verify_soa copies into pinned staging
   first); a batch small enough for the latency kernels (the
   fd_ed25519_amd_set_small_batch_max cap, default 16384, and at most
   batch_max) is read in place by the GPU over PCIe, with no copy at all.
   Same arguments, verdicts and errors as
   fd_ed25519_amd_verify_soa; FD_ED25519_AMD_ERR_INVAL if a plane is not
   registered.  A chunk whose messages are scattered over much more than
   their total size is gathered through the staging instead. */
int
fd_ed25519_amd_host_register( void * base, ulong sz );

int
fd_ed25519_amd_host_unregister( void * base );

int
fd_ed25519_amd_verify_soa_registered( fd_ed25519_amd_t * eng,
                                      ulong              n,
                                      uchar const *      pub,
                                      uchar const *      sig,
                                      uint const *       msg_off,
                                      uint const *       msg_sz,
                                      uchar const *      blob,
                                      ulong              blob_sz,
                                      schar *            err );

/* Pointer-array batch from registered memory: the arguments, verdicts and
   engine mode of fd_ed25519_amd_verify_batch, without its staging.  The
   host copies no record byte: per chunk it writes one 32-B record per
   signature (three device addresses, the size, an offset), and a kernel
   (k_gather) fetches the 32 + 64 + sz bytes over PCIe straight into the
   device planes the verify kernels read.  pub[i], sig[i] and msg[i] may have
   any byte alignment, may repeat and may overlap.

   Requirement: every [pub[i], +32), [sig[i], +64) and non-empty
   [msg[i], +sz[i]) lies inside ONE registration made through
   fd_ed25519_amd_host_register (its first and its last byte in the same
   one; two adjacent registrations do not make one range).  Only that table
   is consulted: memory pinned or registered by other means is refused, as a
   HIP pointer query per signature would cost more than the copy this call
   saves.  msg[i] is not looked at when sz[i] is 0.

   Every argument of every signature is checked before anything launches:
   a NULL array, a NULL pub[i] / sig[i], a NULL msg[i] with sz[i] > 0,
   sz[i] > blob_max, or a range the table does not hold returns
   FD_ED25519_AMD_ERR_INVAL with err (and tag) untouched and nothing in
   flight; this call never gives the GPU an address the table did not
   produce.  (fd_ed25519_amd_submit_frags, fd_tango_amd.h, widens that: there
   every address in a record lies inside one registered data region with its
   whole range, as computed on the device, or is the slot's own idle block.)
   Unregistering memory, or changing the pointer arrays, during the call is
   the caller's error (as for fd_ed25519_amd_verify_soa_registered).  The
   _tag form is declared with the other tagged calls below. */
int
fd_ed25519_amd_verify_batch_registered( fd_ed25519_amd_t *   eng,
                                        ulong                n,
                                        void const * const * msg,
                                        ulong const *        sz,
                                        void const * const * sig,
                                        void const * const * pub,
                                        schar *              err );

/* How fd_ed25519_amd_verify_batch_registered cuts a batch into chunks (pure
   host code, no device): of n signatures with message sizes sz[], one chunk
   takes the first -- always -- and further ones while the count stays <= cap
   (the engine's batch_max) and the padded total, the sum of
   round_up( sz[i], 16 ), stays <= blob_cap (its blob_max).  Returns the
   number taken and writes dst[0 .. that): each message's offset in the
   chunk's device blob, a multiple of 16, ascending. */
ulong
fd_ed25519_amd_gather_layout( ulong n, ulong const * sz, ulong cap, ulong blob_cap, uint * dst );

/* Multi-device engine (SURVEY s8 e: signatures are independent, so a batch
   shards with no exchange step).  One engine and one persistent host thread
   per entry of devices[0..ndev) (a device may be listed more than once:
   several engines share it); a batch is split into contiguous shards, one
   per engine, verified concurrently, and the call returns when every shard
   is done.  No collective, no peer traffic: each shard's inputs go host ->
   its device, its verdicts device -> host.  The reference scales the same
   way, as N independent verify tiles each with its own input
   (src/app/frank/fd_frank_init:67-80).  batch_max / blob_max are per
   engine.  One call at a time per multi engine (its worker threads serve
   one batch at a time); independent multi engines may run concurrently.
   NULL on failure (any device unusable). */
typedef struct fd_ed25519_amd_multi fd_ed25519_amd_multi_t;

fd_ed25519_amd_multi_t *
fd_ed25519_amd_multi_new( int const * devices, ulong ndev, ulong batch_max, ulong blob_max );

void
fd_ed25519_amd_multi_delete( fd_ed25519_amd_multi_t * multi );

ulong
fd_ed25519_amd_multi_ndev( fd_ed25519_amd_multi_t const * multi );

/* fd_ed25519_amd_set_mode on every engine of the multi engine (between
   batches).  FD_ED25519_AMD_OK or FD_ED25519_AMD_ERR_INVAL. */
int
fd_ed25519_amd_multi_set_mode( fd_ed25519_amd_multi_t * multi, int mode );

/* Shard [lo, hi) of n items that engine r of ndev verifies: lo = n*r/ndev. */
void
fd_ed25519_amd_shard_range( ulong n, ulong ndev, ulong r, ulong * lo, ulong * hi );

/* NUMA placement.  Each multi-engine thread binds itself to its device's
   NUMA node (the node's CPUs it may use, and the node as its preferred
   memory) before creating its engine, so the pinned staging it fills is
   node-local; a single engine prefers the device's node while it allocates
   its staging and leaves the caller's thread as it was.
   FD_ED25519_AMD_NUMA=0 turns both off.  The node of a device:
   hipDeviceGetPCIBusId -> /sys/bus/pci/devices/<bdf>/numa_node (-1 when
   unknown).  fd_ed25519_amd_sysfs_numa reads that file and the node's
   cpulist under any sysfs root: node (-1 if unknown) and up to cpus_max
   CPUs; returns the CPU count, -1 on an unreadable or malformed tree. */
int
fd_ed25519_amd_device_numa_node( int device );

int
fd_ed25519_amd_sysfs_numa( char const * sysfs_root, char const * pci_bdf, int * node, int * cpus, int cpus_max );

/* fd_ed25519_amd_verify_soa over the engines (same arguments and
   verdicts; err[i] for every i).  Returns the first engine error, if any. */
int
fd_ed25519_amd_multi_verify_soa( fd_ed25519_amd_multi_t * multi,
                                 ulong                    n,
                                 uchar const *            pub,
                                 uchar const *            sig,
                                 uint const *             msg_off,
                                 uint const *             msg_sz,
                                 uchar const *            blob,
                                 ulong                    blob_sz,
                                 schar *                  err );

/* Dedup tags.  The tile downstream of verify deduplicates on the mcache
   `sig` field, which this project sets to a hash the verify computes anyway:

     tag[i] = the little-endian u64 of bytes 0..7 of
              SHA-512( sig[i][0:32] || pub[i] || msg[i] )

   fd_ed25519_amd_tag is that definition as pure host code (no device; what
   a unit test or a CPU-only caller computes).  Each *_tag batch call below
   is the call it is named after plus `tag`, n entries of caller memory, and
   returns for every signature the value the GPU already hashed:
     - 0 where the engine does not hash: a signature the reference's s check
       rejects (reference verdict FD_ED25519_ERR_SIG);
     - the hash everywhere else: for verdicts 0, -2 and -3, and for an s the
       reference's window accepts without a multiply (reference verdict 0);
     - the same value in both verdict modes: an s-window signature is -1 in
       FD_ED25519_AMD_MODE_STRICT and still carries its hash.
   tag == NULL is exactly the untagged call (nothing more is launched or
   copied); the untagged functions are these with tag == NULL.  Like err,
   tag is written only during the call, and its contents are unspecified
   when the call returns an error.  In-batch duplicates are not filtered by
   these calls: dedup stays the caller's.  (The _keep submissions, "Survivors"
   below, return the filtered list of one submission.) */
ulong
fd_ed25519_amd_tag( void const * msg,
                    ulong        sz,
                    void const * sig,
                    void const * public_key );

int
fd_ed25519_amd_verify_batch_tag( fd_ed25519_amd_t *   eng,
                                 ulong                n,
                                 void const * const * msg,
                                 ulong const *        sz,
                                 void const * const * sig,
                                 void const * const * pub,
                                 schar *              err,
                                 ulong *              tag );

int
fd_ed25519_amd_verify_batch_registered_tag( fd_ed25519_amd_t *   eng,
                                            ulong                n,
                                            void const * const * msg,
                                            ulong const *        sz,
                                            void const * const * sig,
                                            void const * const * pub,
                                            schar *              err,
                                            ulong *              tag );

int
fd_ed25519_amd_verify_soa_tag( fd_ed25519_amd_t * eng,
                               ulong              n,
                               uchar const *      pub,
                               uchar const *      sig,
                               uint const *       msg_off,
                               uint const *       msg_sz,
                               uchar const *      blob,
                               ulong              blob_sz,
                               schar *            err,
                               ulong *            tag );

/* tag (like err) is plain caller memory: it need not be registered. */
int
fd_ed25519_amd_verify_soa_registered_tag( fd_ed25519_amd_t * eng,
                                          ulong              n,
                                          uchar const *      pub,
                                          uchar const *      sig,
                                          uint const *       msg_off,
                                          uint const *       msg_sz,
                                          uchar const *      blob,
                                          ulong              blob_sz,
                                          schar *            err,
                                          ulong *            tag );

/* Every shard writes its tags at its fd_ed25519_amd_shard_range offset. */
int
fd_ed25519_amd_multi_verify_soa_tag( fd_ed25519_amd_multi_t * multi,
                                     ulong                    n,
                                     uchar const *            pub,
                                     uchar const *            sig,
                                     uint const *             msg_off,
                                     uint const *             msg_sz,
                                     uchar const *            blob,
                                     ulong                    blob_sz,
                                     schar *                  err,
                                     ulong *                  tag );

/* ===== Asynchronous submissions =====

   Every batch call above returns when its last chunk has been delivered; a
   caller with a run loop of its own is stuck inside the call for the whole
   GPU round trip.  The submit calls launch ONE chunk on one of the engine's
   slots and return; fd_ed25519_amd_async_poll / fd_ed25519_amd_async_wait
   deliver finished submissions later.  One thread can so keep
   fd_ed25519_amd_async_depth( eng ) submissions in flight (the engine's slot
   count: fd_ed25519_amd_new_slots) and do its other work in between.

   Each submit call takes the arguments of the most general synchronous call
   of its family plus `ticket`:
     fd_ed25519_amd_submit_batch             fd_ed25519_amd_verify_batch_tag
     fd_ed25519_amd_submit_batch_registered  fd_ed25519_amd_verify_batch_registered_tag
     fd_ed25519_amd_submit_txns              fd_ed25519_amd_verify_txns_desc            (fd_txn_amd.h)
     fd_ed25519_amd_submit_txns_registered   fd_ed25519_amd_verify_txns_registered_desc (fd_txn_amd.h)
   Optional outputs are NULL exactly as in the synchronous call.

   One chunk per submission.  A submission must fit the chunk the matching
   synchronous call would cut first: for the registered forms,
   fd_ed25519_amd_gather_layout / fd_ed25519_amd_txn_gather_layout over the
   whole submission returns n; for the staged forms, the count (batch_max),
   signature-slot (batch_max, transactions) and byte (blob_max, unpadded) caps
   of their chunk loops hold for the whole submission.  Otherwise, and for
   n == 0 or ticket == NULL, the submit returns FD_ED25519_AMD_ERR_INVAL.
   Every argument check of the synchronous call applies unchanged, the
   registration table and the descriptor bound included.  On any error return
   nothing is launched, no output is touched, no ticket is consumed and
   *ticket is untouched.

   Tickets are per engine: 1, 2, 3, ..., one per accepted submission.
   Submissions take the slots round robin.

   Busy.  With fd_ed25519_amd_async_depth submissions in flight a submit
   returns FD_ED25519_AMD_ERR_BUSY, with the effect of an error return.  (A
   full engine says BUSY before the one-chunk rule is looked at; the argument
   checks come first.)

   Inputs.  The staged forms copy every input byte during the submit call: the
   caller may reuse or free msg, sig, pub, payload and the index arrays as
   soon as it returns.  The registered forms read the caller's memory until
   delivery: the pointed-to bytes and the registration must stay valid until
   then; the pointer and size arrays themselves are consumed during submit.

   Outputs are written only inside async_poll / async_wait, by the call that
   reports the ticket; until then the caller's output arrays are not touched.
   The one exception is sig_base, pure host numbering, written by the submit
   call.  Outputs are byte for byte those of the synchronous call for the same
   arguments, in the verdict mode the engine had at submit.  Descriptor
   offsets are relative to the submission: desc_off[0] == 0.

   Delivery is in ticket order, one submission per call.
   fd_ed25519_amd_async_poll never blocks: with nothing in flight, or the
   oldest submission not finished, it returns FD_ED25519_AMD_ASYNC_NONE and
   leaves *ticket alone; when the oldest has finished it delivers it, sets
   *ticket and returns FD_ED25519_AMD_OK -- or FD_ED25519_AMD_ERR_DEVICE when
   that submission hit k_dsmp's step guard (below): its outputs are then
   unspecified, and younger submissions are unaffected.
   fd_ed25519_amd_async_wait is the same but blocks for the oldest; it returns
   ASYNC_NONE only when nothing is in flight.  On a HIP runtime error the call
   returns FD_ED25519_AMD_ERR_DEVICE with the oldest ticket, every submission
   in flight is dropped (their outputs are never written) and
   fd_ed25519_amd_async_in_flight becomes 0.

   "Not finished yet" costs one load: the last kernel of a submission
   (k_ticket) stores its ticket into a word of mapped host memory and
   async_poll compares that word; no HIP call is made until it matches.
   Delivery itself still waits for the slot's HIP event, so the outputs never
   depend on the order in which the word and the results become visible.
   FD_ED25519_AMD_ASYNC_POLL=event in the environment when the engine is
   created makes async_poll ask hipEventQuery instead and launches no
   k_ticket (the A/B of tools/async_cost.py).

   Mixing.  While fd_ed25519_amd_async_in_flight( eng ) > 0 every synchronous
   batch call of that engine and fd_ed25519_amd_set_mode return
   FD_ED25519_AMD_ERR_INVAL and touch nothing: they would reuse the slots.
   fd_ed25519_amd_delete waits for what is in flight and delivers nothing.
   The rule stays one engine per host thread: submit, poll and wait of one
   engine come from one thread.

   Out of scope: the SoA shapes (a caller who holds a whole SoA batch gains
   nothing from submitting it in pieces), the multi-device engine, the
   drop-in fd_ed25519_verify and the streaming tile. */
ulong
fd_ed25519_amd_async_depth( fd_ed25519_amd_t const * eng );

ulong
fd_ed25519_amd_async_in_flight( fd_ed25519_amd_t const * eng );

int
fd_ed25519_amd_submit_batch( fd_ed25519_amd_t *   eng,
                             ulong                n,
                             void const * const * msg,
                             ulong const *        sz,
                             void const * const * sig,
                             void const * const * pub,
                             schar *              err,
                             ulong *              tag,
                             ulong *              ticket );

int
fd_ed25519_amd_submit_batch_registered( fd_ed25519_amd_t *   eng,
                                        ulong                n,
                                        void const * const * msg,
                                        ulong const *        sz,
                                        void const * const * sig,
                                        void const * const * pub,
                                        schar *              err,
                                        ulong *              tag,
                                        ulong *              ticket );

int
fd_ed25519_amd_async_poll( fd_ed25519_amd_t * eng, ulong * ticket );

int
fd_ed25519_amd_async_wait( fd_ed25519_amd_t * eng, ulong * ticket );

/* ===== Survivors: in-batch dedup and the verdict filter =====

   What a verify tile publishes is not a verdict per input but the inputs
   that passed and were not seen before.  The _keep submissions return that
   list for one submission, made on the GPU behind the verify kernels, so the
   caller's last O(n) pass per batch (drop the failures, find the duplicates
   with a hash set of its own, build the list to forward) goes away.

   The rule, one definition for every layer.  For n items with verdicts
   err[i] and tags tag[i] ("Dedup tags" above), item i is a survivor iff
     1. err[i] == 0, and
     2. tag[i] == 0, or no j < i has err[j] == 0 and tag[j] == tag[i].
   Tag 0 is never deduplicated (the tile's FD_TCACHE_TAG_NULL rule).  Only
   passing items occupy a tag: the tag is SHA-512( R || A || M ) and does not
   cover s, so a copy with a corrupted s ahead of the valid one does not
   suppress it.  keep[0 .. keep_cnt) holds the survivors' indices, ascending.
   The items are signatures (err, tag) in the signature family and
   transactions (txn_err, txn_tag: the tag of the first signature) in the
   transaction family (fd_txn_amd.h).  The verdicts are those of the engine's
   mode at submit: an s-window signature is a survivor in reference mode and
   not in strict mode.  The dedup window is one submission, which is one
   chunk -- unless the engine has a window attached ("The dedup window"
   below), which carries the tags from one submission to the next.

   fd_ed25519_amd_keep is the rule as pure host code (no device; what a
   CPU-only caller or a unit test computes): it returns keep_cnt and writes
   keep[0, keep_cnt) and nothing else; keep == NULL only counts.

   fd_ed25519_amd_keep_dev is the filter alone, device-resident, with the
   conventions of the other _dev calls (the caller's stream, no sync): d_err
   and d_tag are n entries of device memory (d_tag 8-aligned: what
   fd_ed25519_amd_tags_dev / fd_ed25519_amd_txn_tags_dev produce, so a
   device-resident caller chains the calls it already has); d_keep (n
   entries, 4-aligned) and d_keep_cnt (8-aligned) are device or mapped host
   memory; d_scratch is at least fd_ed25519_amd_keep_scratch_footprint( n )
   bytes of device memory, 256-aligned.  n is at most 2^30 (the footprint of
   a larger n is 0 and the call returns FD_ED25519_AMD_ERR_INVAL).  Memory,
   as for fd_ed25519_amd_verify_dev: the scratch may hold anything on entry;
   the call writes d_scratch[0, footprint( n )), d_keep[0, keep_cnt) and
   *d_keep_cnt and nothing else; d_err and d_tag are only read; n == 0 writes
   *d_keep_cnt = 0 only.  Passing items with a nonzero tag meet in an
   open-addressed table in the scratch (at least 2 n slots); a slot is chosen
   by a 64-bit mix of tag ^ salt.  Tags are hashes an attacker chooses: with
   a known slot function it could grind tags into one probe chain and make
   the filter quadratic, so salt should be a secret (the engine draws its own
   from the OS once, at creation).  No output depends on salt.  Kernels
   ordered by the stream; no workgroup ever waits for another.

   The _keep submissions take the arguments of the submit call they are named
   after plus keep (capacity n / txn_cnt entries) and keep_cnt before ticket.
   Both NULL is exactly that submit call; one without the other is
   FD_ED25519_AMD_ERR_INVAL, with the effect of every error return.
   Everything in "Asynchronous submissions" holds unchanged: one chunk, BUSY,
   the inputs, ticket order, the error returns, the mode at submit,
   FD_ED25519_AMD_ASYNC_POLL.  keep[0, keep_cnt) and *keep_cnt are written at
   delivery, by the poll / wait that reports the ticket; no byte of keep at or
   beyond keep_cnt is written.  The tags the filter needs are produced on the
   device whether or not the caller asked for tag; every other output (err,
   tag) is what the plain submit delivers, for all n items.  The slot's
   buffers for the filter are allocated by the first submission that asks.

   Out of scope: the synchronous multi-chunk calls and the SoA shapes (a
   dedup window over several chunks needs the inserts of different streams
   ordered), the multi-device engine, the streaming tile (which has its own
   dedup) and the drop-in fd_ed25519_verify.  Dedup across submissions is
   the window's, below. */
ulong
fd_ed25519_amd_keep( ulong         n,
                     schar const * err,
                     ulong const * tag,
                     uint *        keep );

ulong
fd_ed25519_amd_keep_scratch_footprint( ulong n );

int
fd_ed25519_amd_keep_dev( ulong         n,
                         schar const * d_err,
                         ulong const * d_tag,
                         uint *        d_keep,
                         ulong *       d_keep_cnt,
                         void *        d_scratch,
                         ulong         salt,
                         void *        stream );

int
fd_ed25519_amd_submit_batch_keep( fd_ed25519_amd_t *   eng,
                                  ulong                n,
                                  void const * const * msg,
                                  ulong const *        sz,
                                  void const * const * sig,
                                  void const * const * pub,
                                  schar *              err,
                                  ulong *              tag,
                                  uint *               keep,
                                  ulong *              keep_cnt,
                                  ulong *              ticket );

int
fd_ed25519_amd_submit_batch_registered_keep( fd_ed25519_amd_t *   eng,
                                             ulong                n,
                                             void const * const * msg,
                                             ulong const *        sz,
                                             void const * const * sig,
                                             void const * const * pub,
                                             schar *              err,
                                             ulong *              tag,
                                             uint *               keep,
                                             ulong *              keep_cnt,
                                             ulong *              ticket );

/* ===== Output frames: the survivors' bytes, written by the GPU =====

   A tile that reads from an input link publishes from a dcache of its own,
   so after a _keep submission its thread would still copy every survivor
   into that dcache.  The _emit submissions have the GPU do it: the calling
   thread does one fd_mcache_publish per survivor and touches no payload
   byte.

   The rule (one definition, shared by every layer).  A submission's
   survivors are keep[0, keep_cnt), as above, window included.  For survivor
   j, item i = keep[j], a FRAME of emit_sz[j] bytes is written at
   out + emit_off[j]:
   - signature family: pub[i] (32) | sig[i] (64) | msg[i] (sz[i]), so
     emit_sz = 96 + sz[i] -- the frag layout the streaming tile takes in;
   - transaction family (fd_txn_amd.h): payload (P = txn_sz[i]) | zero bytes
     up to P16 = round_up( P, 16 ) | fd_txn_t (F = its footprint, even) | P
     as a little-endian u16, so emit_sz = P16 + F + 2.  A consumer reads P
     from the frame's last two bytes; the descriptor starts at the 16-aligned
     offset round_up( P, 16 ), so a cast to fd_txn_t * is legal; its bytes
     are the ones fd_txn_parse writes, that is, what the _desc calls return.
   - placement: emit_off[0] = 0, emit_off[j+1] = emit_off[j] +
     round_up( emit_sz[j], 128 ) -- the stride of fd_dcache_compact_next,
     without its wrap.  emit_off has keep_cnt + 1 defined entries, the last
     one the total.  Survivor j is published with chunk = chunk_of( out ) +
     ( emit_off[j] >> 6 ) and sz = emit_sz[j].
   - bytes written: exactly [ emit_off[j], emit_off[j] + round_up(
     emit_sz[j], 16 ) ) per frame, the frame and then zeros.  No other byte of
     out, and nothing outside it, is written.
   Each submission gets an extent of its own from the caller; there is no
   cursor shared between submissions and no new ordering among streams.  The
   caller decides where its ring wraps.

   Pure host code (no device): fd_ed25519_amd_emit_bound( msg_sz ) =
   round_up( 96 + msg_sz, 128 ), at least the stride of any such frame.
   fd_ed25519_amd_emit is the rule for the signature family over pointer
   arrays, as the batch calls take them: it returns the total byte count and
   writes emit_off[0, keep_cnt], emit_sz[0, keep_cnt) and the frames; out ==
   NULL only computes the layout; a total above out_cap returns ~0UL and
   writes nothing.  It is what a CPU-only caller runs and what the tests
   check the GPU against.

   fd_ed25519_amd_emit_dev is the step alone, device-resident, with the
   conventions of fd_ed25519_amd_keep_dev (the caller's stream, no sync, the
   scratch's contents irrelevant).  The inputs are the verify planes and a
   publish list in d_keep / d_keep_cnt, so a device-resident caller chains the
   calls it already has.  d_out: 64-aligned, device or mapped host memory;
   d_emit_off (8-aligned, n + 1 entries) and d_emit_sz (n entries): device or
   mapped host memory; d_scratch: fd_ed25519_amd_emit_scratch_footprint( n )
   bytes of device memory, 256-aligned (n at most 2^30; beyond, the footprint
   is 0 and the call FD_ED25519_AMD_ERR_INVAL).  Capacity follows
   fd_txn_amd_parse_packed_dev's rule: frame j is stored only if
   emit_off[j+1] <= out_cap, otherwise none of it is, and d_emit_off is
   complete either way.  Bounded reads and writes: *d_keep_cnt is clamped to
   n; an index >= n (or an item too large for a frame: a message above
   2^32 - 4192 bytes) emits a frame of size 0 and reads nothing; no contents
   of d_keep cause a read or a store out of bounds.  Writes d_emit_off[0,
   cnt], d_emit_sz[0, cnt), the frames and the scratch, nothing else.  The
   capacity is checked on the device before any store of a frame.

   The _emit submissions take the arguments of their _keep form with out,
   out_cap, emit_off (capacity n + 1) and emit_sz (capacity n) in front of
   ticket.  All four NULL / 0 is exactly the _keep call: nothing more is
   launched or allocated.  FD_ED25519_AMD_ERR_INVAL, with the effect of every
   error return: any one of the four without the others; emit without keep;
   out not 64-aligned; [out, out + out_cap) not inside ONE registration of
   fd_ed25519_amd_host_register (only that table is consulted; two adjacent
   registrations do not make one range); out_cap below the sum of the bound
   over all items of the submission -- the capacity is decided by the bound,
   never by the data.  The GPU writes the extent between submit and
   delivery: the caller leaves it alone and keeps it registered until then,
   and overlapping extents of two submissions in flight are the caller's
   error.  emit_off[0, keep_cnt] and emit_sz[0, keep_cnt) are written by the
   poll or wait that reports the ticket, nothing beyond them, and the frames
   are complete by then.  After FD_ED25519_AMD_ERR_DEVICE the extent's
   contents are unspecified, inside its bounds.  With a window attached the
   frames are the window's survivors'; the emit step runs behind the filter,
   outside the stretch that is serial among submissions.  The verdict mode
   matters only through keep.  Every other output is the _keep call's.  The
   slot's buffers are allocated by the first submission that asks.  Out of
   scope, as for _keep: the blocking calls, the SoA shapes, the multi-device
   engine, the streaming tile and the drop-in. */
ulong
fd_ed25519_amd_emit_bound( ulong msg_sz );

ulong
fd_ed25519_amd_emit( ulong                keep_cnt,
                     uint const *         keep,
                     void const * const * msg,
                     ulong const *        sz,
                     void const * const * sig,
                     void const * const * pub,
                     void *               out,
                     ulong                out_cap,
                     ulong *              emit_off,
                     uint *               emit_sz );

ulong
fd_ed25519_amd_emit_scratch_footprint( ulong n );

int
fd_ed25519_amd_emit_dev( ulong         n,
                         uchar const * d_pub,
                         uchar const * d_sig,
                         uint const *  d_msg_off,
                         uint const *  d_msg_sz,
                         uchar const * d_blob,
                         uint const *  d_keep,
                         ulong const * d_keep_cnt,
                         void *        d_out,
                         ulong         out_cap,
                         ulong *       d_emit_off,
                         uint *        d_emit_sz,
                         void *        d_scratch,
                         void *        stream );

int
fd_ed25519_amd_submit_batch_emit( fd_ed25519_amd_t *   eng,
                                  ulong                n,
                                  void const * const * msg,
                                  ulong const *        sz,
                                  void const * const * sig,
                                  void const * const * pub,
                                  schar *              err,
                                  ulong *              tag,
                                  uint *               keep,
                                  ulong *              keep_cnt,
                                  void *               out,
                                  ulong                out_cap,
                                  ulong *              emit_off,
                                  uint *               emit_sz,
                                  ulong *              ticket );

int
fd_ed25519_amd_submit_batch_registered_emit( fd_ed25519_amd_t *   eng,
                                             ulong                n,
                                             void const * const * msg,
                                             ulong const *        sz,
                                             void const * const * sig,
                                             void const * const * pub,
                                             schar *              err,
                                             ulong *              tag,
                                             uint *               keep,
                                             ulong *              keep_cnt,
                                             void *               out,
                                             ulong                out_cap,
                                             ulong *              emit_off,
                                             uint *               emit_sz,
                                             ulong *              ticket );

/* ===== The dedup window: dedup across submissions =====

   A window remembers the last `depth` tags its caller published, in device
   memory, so that the _keep submissions of an engine it is attached to drop
   what an EARLIER submission already delivered: keep[] is then what a verify
   tile forwards, and the caller keeps no tag cache of its own.  The
   reference's verify and dedup tiles keep an fd_tcache for this
   (src/tango/tcache/fd_tcache.h:372-403).

   The rule, one definition for every layer.  A window has a depth D >= 1 and
   the sequence T[0..H) of every tag it ever inserted (H a 64-bit count).  Its
   LIVE tags at H are T[q] for max( 0, H - D ) <= q < H; they are distinct by
   construction.  One submission of n <= D items (err[i], tag[i]) acts on the
   window as it stands WHEN THE SUBMISSION STARTS:
     - item i is a survivor iff err[i] == 0, and tag[i] == 0 or no j < i has
       err[j] == 0 and tag[j] == tag[i] (the rule of "Survivors"), and tag[i]
       is not live;
     - afterwards the survivors with a nonzero tag are appended to T in
       ascending i, and H grows by their number.
   Tag 0 and failing items are never inserted.  Submissions act on the window
   in ticket order, however they overlap on the GPU and whenever they are
   polled.

   Relation to FD_TCACHE_INSERT applied item by item.  The window is queried
   as of the submission's start, so a tag the submission's own inserts would
   have evicted still counts as a duplicate inside that submission: the
   effective depth is between D and D + n - 1, and no item a depth-D tcache
   with the same history would drop is kept.  The two are equal exactly, keep
   lists and state, whenever no tag evicted during a submission sits on a
   passing item of that same submission.  The item-by-item rule is not the
   rule here because it has a serial dependency: whether item i evicts the
   oldest tag depends on how many earlier items survived, and a GPU decides
   all items of a batch at once.

   fd_ed25519_amd_window_new: a window of `depth` tags (1 ..
   FD_ED25519_AMD_WINDOW_DEPTH_MAX) on HIP device `device`; device < 0 makes
   a host-only window (no HIP call).  salt is the secret of the window's
   table, as for fd_ed25519_amd_keep_dev; 0 draws one from the OS.  No output
   depends on it.  NULL on failure.  Device memory: 8 depth bytes of ring and
   16 bytes for each of the table's slots, whose number is the power of two
   >= max( 4 depth, 256 ): between 72 and 136 bytes per tag of depth, 264 MiB
   at the largest depth.  fd_ed25519_amd_window_delete waits for the window's
   queued work and detaches it from its engine.

   fd_ed25519_amd_window_keep is the rule as pure host code on a host-only
   window (what a CPU-only caller or a unit test computes, and the tag cache
   a caller would otherwise keep behind a windowless engine): it returns
   keep_cnt and writes keep[0, keep_cnt) only (keep == NULL only counts).
   n > depth, or a device window, returns ~0UL and changes nothing.

   fd_ed25519_amd_window_keep_dev is the filter alone, device-resident, with
   fd_ed25519_amd_keep_dev's conventions and arguments (the table salt is the
   window's): d_scratch is at least
   fd_ed25519_amd_window_keep_scratch_footprint( n ) bytes (the filter's
   planes, then a second flag plane and its scan: about 4.2 n bytes more).
   The caller orders the calls on one window: the same stream, or events.
   n == 0 writes *d_keep_cnt = 0 only and leaves the window alone.  n > depth,
   a host-only window, or a window attached to an engine returns
   FD_ED25519_AMD_ERR_INVAL and enqueues nothing.

   fd_ed25519_amd_window_export returns cnt <= depth and writes the live tags
   to tags[0, cnt), oldest first (tags == NULL only counts); it waits for the
   window's queued work; ~0UL on a HIP error.  fd_ed25519_amd_window_import
   replaces the contents with tags[0, cnt), oldest first: cnt <= depth, every
   tag nonzero and distinct; cnt == 0 is a reset.  It waits, too, and is
   refused (ERR_INVAL) while the window's engine has submissions in flight.
   Together they are the clean-restart hook fd_tcache has (oldest_laddr).

   fd_ed25519_amd_set_window: the engine borrows the window; NULL detaches it
   (deleting either object detaches, too).  FD_ED25519_AMD_ERR_INVAL while
   submissions are in flight, for a window of another device (a host-only one
   included), for depth < the engine's batch_max, and for a window attached
   to another engine.  fd_ed25519_amd_window: the engine's window, or NULL.

   With a window attached the four _keep submit forms follow the rule above
   instead of "Survivors" alone; the signature and the transaction forms
   share the window (a transaction's tag is its first signature's).  In the
   transaction forms the descriptors are packed for the window's survivors
   only.  Every other output is unchanged.  Plain submissions, _keep forms
   with keep == NULL and the blocking calls never touch the window; without a
   window every call is what it was.  The window does not depend on the
   verdict mode.  A slot's stream waits for the event the previous _keep
   submission recorded behind its window step, ahead of its own; the verify
   kernels ahead of that point still overlap.  After a submission ends in
   FD_ED25519_AMD_ERR_DEVICE the window's contents are undefined until an
   import. */
#define FD_ED25519_AMD_WINDOW_DEPTH_MAX (1UL<<22)

typedef struct fd_ed25519_amd_window_s fd_ed25519_amd_window_t;

fd_ed25519_amd_window_t *
fd_ed25519_amd_window_new( int device, ulong depth, ulong salt );

void
fd_ed25519_amd_window_delete( fd_ed25519_amd_window_t * win );

ulong
fd_ed25519_amd_window_depth( fd_ed25519_amd_window_t const * win );

ulong
fd_ed25519_amd_window_keep( fd_ed25519_amd_window_t * win,
                            ulong                     n,
                            schar const *             err,
                            ulong const *             tag,
                            uint *                    keep );

ulong
fd_ed25519_amd_window_keep_scratch_footprint( ulong n );

int
fd_ed25519_amd_window_keep_dev( fd_ed25519_amd_window_t * win,
                                ulong                     n,
                                schar const *             d_err,
                                ulong const *             d_tag,
                                uint *                    d_keep,
                                ulong *                   d_keep_cnt,
                                void *                    d_scratch,
                                void *                    stream );

ulong
fd_ed25519_amd_window_export( fd_ed25519_amd_window_t * win, ulong * tags );

int
fd_ed25519_amd_window_import( fd_ed25519_amd_window_t * win, ulong const * tags, ulong cnt );

int
fd_ed25519_amd_set_window( fd_ed25519_amd_t * eng, fd_ed25519_amd_window_t * win );

fd_ed25519_amd_window_t *
fd_ed25519_amd_window( fd_ed25519_amd_t const * eng );

/* Device-resident batch: every pointer is HIP device memory, already
   resident (the layout of fd_ed25519_amd_verify_soa).  Enqueues the
   verify kernels on `stream` (hipStream_t, NULL = default stream) and
   returns without synchronising.  `ws` is device scratch of at least
   fd_ed25519_amd_workspace_footprint(n) bytes, 256-aligned.

   Contract on memory (tests/test_workspace_state_gpu.py; the plane table
   is in DESIGN.md s2): the workspace may hold anything on entry -- the
   leftovers of a launch with another n, kernel or mode, or arbitrary bytes
   -- and no result depends on it: every plane element a kernel reads was
   written earlier in the same call.  The call writes ws[0, footprint(n)),
   d_err[0, n) -- every entry, whatever it held -- and nothing else; the
   input planes (d_pub, d_sig, d_msg_off, d_msg_sz, d_blob) are only read.
   The read-back calls below (work_stats, tags, debug_*) write the n
   entries of their named output and nothing else, and do not write the
   workspace.  One workspace serves one call at a time; calls in flight on
   different streams need workspaces of their own. */
ulong
fd_ed25519_amd_workspace_footprint( ulong n );

int
fd_ed25519_amd_verify_dev( ulong         n,
                           uchar const * d_pub,
                           uchar const * d_sig,
                           uint const *  d_msg_off,
                           uint const *  d_msg_sz,
                           uchar const * d_blob,
                           schar *       d_err,
                           void *        d_ws,
                           void *        stream );

/* Same as fd_ed25519_amd_verify_dev; when ev != NULL it points to 4
   hipEvent_t that are recorded on `stream` before k_prep, between the
   stages and after k_dsm (per-stage kernel timing for the bench). */
int
fd_ed25519_amd_verify_dev_ev( ulong         n,
                              uchar const * d_pub,
                              uchar const * d_sig,
                              uint const *  d_msg_off,
                              uint const *  d_msg_sz,
                              uchar const * d_blob,
                              schar *       d_err,
                              void *        d_ws,
                              void *        stream,
                              void * const * ev );

/* The two calls above with the verdict mode as an argument (there is no
   engine to carry it): FD_ED25519_AMD_MODE_REFERENCE is the call above,
   FD_ED25519_AMD_MODE_STRICT also enqueues the strict overlay kernel after
   the double-scalar-multiply stage (before ev[3]), which rewrites d_err
   with the strict verdicts.  Same workspace.  Any other mode:
   FD_ED25519_AMD_ERR_INVAL, checked first, nothing is enqueued. */
int
fd_ed25519_amd_verify_dev_mode( ulong         n,
                                uchar const * d_pub,
                                uchar const * d_sig,
                                uint const *  d_msg_off,
                                uint const *  d_msg_sz,
                                uchar const * d_blob,
                                schar *       d_err,
                                void *        d_ws,
                                void *        stream,
                                int           mode );

int
fd_ed25519_amd_verify_dev_ev_mode( ulong         n,
                                   uchar const * d_pub,
                                   uchar const * d_sig,
                                   uint const *  d_msg_off,
                                   uint const *  d_msg_sz,
                                   uchar const * d_blob,
                                   schar *       d_err,
                                   void *        d_ws,
                                   void *        stream,
                                   void * const * ev,
                                   int           mode );

/* Optional per-signature work statistics of the last device-resident call
   on the same workspace: d_stats is planar [3][n] uint (double-scalar-
   multiply loop iterations, nonzero h digits, nonzero s digits; zeros for
   signatures decided before the multiply) -- used to report the
   algorithmic multiply count.  Enqueued on `stream`. */
int
fd_ed25519_amd_work_stats_dev( ulong n, void const * d_ws, uint * d_stats, void * stream );

/* The dedup tags (above) of the last device-resident call on the same
   workspace, in either mode: d_tag[i], n entries of device memory (or
   mapped host memory), 8-aligned.  Tags are not arguments of the
   fd_ed25519_amd_verify_dev* calls: the verify leaves them in the
   workspace and this reads them back.  Enqueued on `stream`, no sync. */
int
fd_ed25519_amd_tags_dev( ulong n, void const * d_ws, ulong * d_tag, void * stream );

/* Debug: copy the signed sliding-window digits (u16 [n][256], low byte =
   digit of h = SHA-512(R||A||M) mod L, high byte = digit of s; recoding of
   avx/fd_ed25519_ge.c:378-400) and the top digit position (int [n]) that
   the last device-resident call left in workspace `d_ws`. */
int
fd_ed25519_amd_debug_digits_dev( ulong n, void const * d_ws, unsigned short * d_dig, int * d_top, void * stream );

/* Debug: copy the decompression's output that the last device-resident
   call left in workspace `d_ws`: d_A int [30][n] (-A.X, A.Y, -A.T limbs;
   A.Z == 1), d_R int [20][n] (R.X, R.Y limbs), d_ds uchar [n][2]
   (decompression status of A / R: 0 ok, 1 not on the curve; limbs are
   valid only where the status is 0 and the s check passed).  Reference:
   avx/fd_ed25519_ge.c:221-299 and the negation of user.c:406-407. */
int
fd_ed25519_amd_debug_points_dev( ulong n, void const * d_ws, int * d_A, int * d_R, unsigned char * d_ds, void * stream );

/* Host-side batch keygen + sign over the SoA layout (workload synthesis;
   not the verify path): prv[n][32] -> pub[n][32], sig[n][64] over
   blob[msg_off[i] .. +msg_sz[i]), on nthread host threads.  Returns 0. */
int
fd_ed25519_amd_sign_batch( ulong         n,
                           uchar const * prv,
                           uchar const * blob,
                           uint const *  msg_off,
                           uint const *  msg_sz,
                           uchar *       pub,
                           uchar *       sig,
                           int           nthread );

/* GPU batch keygen + sign (workload synthesis): device
   buffers prv[n][32] (32-aligned records), messages d_blob[d_msg_off[i] ..
   +d_msg_sz[i]) -> d_pub[n][32], d_sig[n][64]; the bytes equal
   fd_ed25519_public_from_private / fd_ed25519_sign (deterministic RFC 8032).
   Not constant time: never for real keys.  Enqueued on `stream`. */
int
fd_ed25519_amd_sign_dev( ulong         n,
                         uchar const * d_prv,
                         uint const *  d_msg_off,
                         uint const *  d_msg_sz,
                         uchar const * d_blob,
                         uchar *       d_pub,
                         uchar *       d_sig,
                         void *        stream );

/* Kernel choice for the double-scalar multiply, by batch size.  Batches
   of at most fd_ed25519_amd_set_latency_batch_max signatures (default 8192)
   run k_dsm8 (eight lanes per signature: the shortest per-batch latency
   while its waves fit one per SIMD); batches of at most
   fd_ed25519_amd_set_small_batch_max (default 16384) run k_dsm4 (four lanes
   per signature); larger ones the throughput kernel k_dsm (one lane per
   signature, its own op per lane), or k_dsmp (one lane per signature,
   signatures pooled per wave so that a wave runs one op class at a time)
   for batches of at least fd_ed25519_amd_set_pool_batch_min signatures
   (default 2^19; ~0UL disables it).  All give identical verdicts; 0
   disables a latency kernel.  Process-wide. */
void
fd_ed25519_amd_set_small_batch_max( ulong n );

void
fd_ed25519_amd_set_latency_batch_max( ulong n );

void
fd_ed25519_amd_set_pool_batch_min( ulong n );

/* k_dsmp bounds its step loop (a hang guard: every step advances at least
   one op of a signature's bounded op stream).  If a launch ever reaches the
   bound, every verdict of that launch is set to FD_ED25519_AMD_VERDICT_DEVICE
   (never a reference code) and the host batch calls return
   FD_ED25519_AMD_ERR_DEVICE instead of verdicts; device-resident callers
   (fd_ed25519_amd_verify_dev) see the marker in d_err.  Debug: cap the
   bound at `cap` steps per wave (0 restores it), to exercise that path. */
#define FD_ED25519_AMD_VERDICT_DEVICE (-128)
void
fd_ed25519_amd_debug_set_pool_iter_cap( ulong cap );

/* Debug: k_dsmp's grid.  By default a batch of n launches min( ceil(n/64),
   8 per CU ) waves, each holding a pool of 112 signatures, so below
   64 * 8 * CUs signatures no wave ever refills a slot a finished signature
   freed.  w > 0 launches min( w, 8 per CU ) waves whatever n is (tests: one
   or a few waves working through a small batch, every slot reused); 0
   restores the policy.  Launch code only; verdicts do not depend on it.
   Process-wide. */
void
fd_ed25519_amd_debug_set_pool_waves( ulong w );

/* Debug: the double-scalar multiply's output R' = [s]B - [h]A that the last
   device-resident call left parked in workspace `d_ws`, read through the
   parking layout of DSM kernel `kind` (the loaders strict mode uses): d_xyz
   int [30][n], the limbs of X | Y | Z (a projective point; reference:
   avx/fd_ed25519_ge.c:408-527, the operands of the compare at
   user.c:417-425).  kind names the kernel that ran: FD_ED25519_AMD_DSM_K_*,
   or FD_ED25519_AMD_DSM_DEFAULT for the one the batch-size rule above gives
   n signatures under the thresholds set now (the same function chooses the
   kernel at launch).  A row is defined only for a signature whose multiply
   ran: one that passed the s check (not -1, not the s window's early 0) and
   whose A and R decoded (not -2); the other rows hold unspecified values.
   Not defined after the step guard tripped.  Enqueued on `stream`. */
#define FD_ED25519_AMD_DSM_DEFAULT (0)
#define FD_ED25519_AMD_DSM_K_DSM   (1)
#define FD_ED25519_AMD_DSM_K_DSM4  (2)
#define FD_ED25519_AMD_DSM_K_DSM8  (3)
#define FD_ED25519_AMD_DSM_K_DSMP  (4)
int
fd_ed25519_amd_debug_rprime_dev( ulong n, void const * d_ws, int kind, int * d_xyz, void * stream );

/* Debug: where the planes of an n-signature workspace lie (pure host code,
   no device): out[0] = N, the row count (n rounded up to 64, at least 64);
   out[1..11] = the byte offsets of the planes dig, evn, top, A, R, Ai, st,
   tag, ds, init, ctr, in this order; out[12] =
   fd_ed25519_amd_workspace_footprint( n ).  The FD_ED25519_AMD_WS_* names
   index out.  Plane sizes in bytes: dig 256 N, evn 4 N, top 4 N, A 120 N,
   R 80 N, Ai 1536 N, st 12 N, tag 8 N, ds 2 N, init 16 N, ctr 16; every
   offset is a multiple of 256.  out == NULL does nothing. */
#define FD_ED25519_AMD_WS_N          (0)
#define FD_ED25519_AMD_WS_DIG        (1)
#define FD_ED25519_AMD_WS_EVN        (2)
#define FD_ED25519_AMD_WS_TOP        (3)
#define FD_ED25519_AMD_WS_A          (4)
#define FD_ED25519_AMD_WS_R          (5)
#define FD_ED25519_AMD_WS_AI         (6)
#define FD_ED25519_AMD_WS_ST         (7)
#define FD_ED25519_AMD_WS_TAG        (8)
#define FD_ED25519_AMD_WS_DS         (9)
#define FD_ED25519_AMD_WS_INIT       (10)
#define FD_ED25519_AMD_WS_CTR        (11)
#define FD_ED25519_AMD_WS_TOTAL      (12)
#define FD_ED25519_AMD_WS_LAYOUT_CNT (13)
void
fd_ed25519_amd_debug_ws_layout( ulong n, ulong * out );

/* Library version / build string. */
char const *
fd_ed25519_amd_version( void );

#ifdef __cplusplus
}
#endif

#endif /* HEADER_fd_ed25519_amd_h */
