#ifndef HEADER_fd_txn_amd_h
#define HEADER_fd_txn_amd_h

/* Solana transaction descriptor types and the GPU transaction front end of
 * the MI355X verify engine.
 *
 * Part 1 is the reference's parsed-transaction layout
 * (src/ballet/txn/fd_txn.h:1-393), reproduced byte for byte so that a
 * descriptor written by the GPU parser (k_txn_parse) is memcmp-equal to the
 * one the reference's fd_txn_parse (src/ballet/txn/fd_txn_parse.c:6-217)
 * writes for the same payload.  When the reference's own fd_txn.h has been
 * included first its definitions are used instead.
 *
 * Part 2 declares the batch entry points: device-side parsing of a batch of
 * wire-format transactions and multi-signer verification of every signature
 * (signature i is checked with public key acct_addr[i] over the message
 * payload[message_off, payload_sz), fd_txn.h:159-217).
 */

#include "fd_ed25519_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ===== Part 1: reference layout (src/ballet/txn/fd_txn.h) ===== */

#ifndef HEADER_fd_src_ballet_txn_fd_txn_h

typedef unsigned short ushort;

#define FD_TXN_VLEGACY               ((uchar)0xFF)   /* fd_txn.h:36 */
#define FD_TXN_V0                    ((uchar)0x00)   /* fd_txn.h:40 */
#define FD_TXN_SIGNATURE_SZ          (64UL)
#define FD_TXN_PUBKEY_SZ             (32UL)
#define FD_TXN_ACCT_ADDR_SZ          (32UL)
#define FD_TXN_BLOCKHASH_SZ          (32UL)
#define FD_TXN_SIG_MAX               (127UL)         /* fd_txn.h:70 */
#define FD_TXN_ACCT_ADDR_MAX         (256UL)
#define FD_TXN_ADDR_TABLE_LOOKUP_MAX (254UL)
#define FD_TXN_INSTR_MAX             (65535UL)
#define FD_TXN_MAX_SZ                (3570UL)        /* fd_txn.h:95 */

struct fd_txn_instr {                                /* fd_txn.h:107-139 */
  uchar  program_id;
  uchar  _padding_reserved_1;
  ushort acct_cnt;
  ushort data_sz;
  ushort acct_off;
  ushort data_off;
};
typedef struct fd_txn_instr fd_txn_instr_t;

struct fd_txn {                                      /* fd_txn.h:146-272 */
  uchar          transaction_version;
  uchar          signature_cnt;
  ushort         signature_off;
  ushort         message_off;
  uchar          readonly_signed_cnt;
  uchar          readonly_unsigned_cnt;
  ushort         acct_addr_cnt;
  ushort         acct_addr_off;
  ushort         recent_blockhash_off;
  uchar          addr_table_lookup_cnt;
  uchar          addr_table_adtl_writable_cnt;
  uchar          addr_table_adtl_cnt;
  uchar          _padding_reserved_1;
  ushort         instr_cnt;
  fd_txn_instr_t instr[];
};
typedef struct fd_txn fd_txn_t;

struct fd_txn_acct_addr_lut {                        /* fd_txn.h:281-318 */
  ushort addr_off;
  uchar  writable_cnt;
  uchar  readonly_cnt;
  ushort writable_off;
  ushort readonly_off;
};
typedef struct fd_txn_acct_addr_lut fd_txn_acct_addr_lut_t;

#define FD_TXN_PARSE_COUNTERS_RING_SZ (32UL)         /* fd_txn.h:322-341 */
struct fd_txn_parse_counters {
  ulong success_cnt;
  ulong failure_cnt;
  ulong failure_ring[ FD_TXN_PARSE_COUNTERS_RING_SZ ];
};
typedef struct fd_txn_parse_counters fd_txn_parse_counters_t;

/* fd_txn.h:369-375 */
static inline ulong
fd_txn_footprint( ulong instr_cnt, ulong addr_table_lookup_cnt ) {
  return sizeof(fd_txn_t) + instr_cnt*sizeof(fd_txn_instr_t) + addr_table_lookup_cnt*sizeof(fd_txn_acct_addr_lut_t);
}

/* fd_txn.h:351-354 */
static inline fd_txn_acct_addr_lut_t *
fd_txn_get_address_tables( fd_txn_t * txn ) {
  return (fd_txn_acct_addr_lut_t *)(txn->instr + txn->instr_cnt);
}

#endif /* HEADER_fd_src_ballet_txn_fd_txn_h */

/* ===== Part 2: GPU transaction batch (new) ===== */

/* Transaction verdict codes.  0 and the FD_ED25519_ERR_* codes keep their
   meaning (the code of the FIRST signature, in signature order, that failed);
   a payload that fd_txn_parse rejects gets FD_TXN_AMD_ERR_PARSE and none of
   its signatures is checked. */
#define FD_TXN_AMD_ERR_PARSE (-4)

/* Device-side batch parse: transaction t is d_payload[d_txn_off[t] ..
   +d_txn_sz[t]).  Writes d_footprint[t] = what fd_txn_parse returns (0 on
   failure, else fd_txn_footprint) and, when d_out != NULL, the fd_txn_t
   descriptor to d_out + t*out_stride (out_stride >= FD_TXN_MAX_SZ, multiple
   of 2).  Enqueued on `stream`; returns 0 or FD_ED25519_AMD_ERR_*.

   Payloads are not capped at the MTU here: like the reference's
   fd_txn_parse, the parser accepts any well-formed payload of up to 65535
   bytes.  FD_TXN_MAX_SZ = 3570 is the largest footprint of a payload of at
   most FD_TXN_AMD_MTU = 1232 bytes only (fd_txn.h:88-92).  The worst case
   is a legacy payload with one signature, two account addresses (the fee
   payer and a program: an instruction's program index must be >= 1) and
   nothing but empty 3-byte instructions: 1 signature count + 64 signature
   + 3 header + 1 account count + 64 accounts + 32 blockhash + 2 instruction
   count = 167 bytes leave (1232 - 167) / 3 = 355 instructions, and
   sizeof(fd_txn_t) + 355*sizeof(fd_txn_instr_t) = 20 + 10*355 = 3570.  The
   same shape at 65535 bytes (the count then takes 3 bytes: 168) holds
   (65535 - 168) / 3 = 21789 instructions, footprint 20 + 10*21789 = 217910;
   no payload's footprint exceeds FD_TXN_AMD_FOOTPRINT_MAX.

   Nothing is ever written outside [d_out + t*out_stride, + out_stride):
   the 20-byte header always fits, and an instruction or lookup-table record
   is stored only if it ends at or before out_stride.  d_footprint[t] stays
   the reference's value, so d_footprint[t] > out_stride says that the
   descriptor of t holds the header and the leading records that fit, not
   the whole of it; a caller that wants every descriptor whole for payloads
   above the MTU uses out_stride = FD_TXN_AMD_FOOTPRINT_MAX.  The records
   are stored while the payload is walked, so the row of a rejected payload
   (d_footprint[t] == 0) holds unspecified bytes, within the same bound. */
#define FD_TXN_AMD_PAYLOAD_MAX   (65535UL)   /* fd_txn_parse.c:73 */
#define FD_TXN_AMD_FOOTPRINT_MAX (20UL + 10UL*(FD_TXN_AMD_PAYLOAD_MAX/3UL) + 8UL*254UL)   /* 220502: every
                                    instruction takes >= 3 payload bytes, at most 254 lookup tables */
int
fd_txn_amd_parse_dev( ulong         txn_cnt,
                      uchar const * d_payload,
                      uint const *  d_txn_off,
                      uint const *  d_txn_sz,
                      uint *        d_footprint,
                      uchar *       d_out,
                      ulong         out_stride,
                      void *        stream );

/* Host batch of wire-format transactions (same layout, host memory):
   parse on the GPU, verify every signature of every well-formed
   transaction with the multi-signer rule, reduce to one verdict per
   transaction.  txn_err[t] in {0, -1, -2, -3, FD_TXN_AMD_ERR_PARSE}.
   Optional outputs (NULL to skip): sig_base[t] = index of transaction t's
   first signature in sig_err (sig_base[txn_cnt] = total signatures) and
   sig_err[...] = per-signature fd_ed25519_verify codes (capacity: the
   total that fd_ed25519_amd_txn_slots returns for the same batch).  Every
   payload must be at most FD_TXN_AMD_MTU bytes (the wire limit), fit the
   engine's blob_max, and reserve at most batch_max signature slots
   (FD_ED25519_AMD_ERR_INVAL otherwise, checked before anything is
   launched; batch_max >= 19 admits every payload).  Returns
   FD_ED25519_AMD_OK or a negative FD_ED25519_AMD_ERR_*. */
#define FD_TXN_AMD_MTU (1232UL)
int
fd_ed25519_amd_verify_txns( fd_ed25519_amd_t * eng,
                            ulong              txn_cnt,
                            uchar const *      payload,
                            uint const *       txn_off,
                            uint const *       txn_sz,
                            ulong              payload_sz,
                            schar *            txn_err,
                            uint *             sig_base,
                            schar *            sig_err );

/* Multi-device form (fd_ed25519_amd_multi_new): the transactions are split
   into contiguous shards, one per device, verified concurrently, each by
   its own engine and host thread; outputs as fd_ed25519_amd_verify_txns,
   sig_base numbered over the whole batch. */
int
fd_ed25519_amd_multi_verify_txns( fd_ed25519_amd_multi_t * multi,
                                  ulong                    txn_cnt,
                                  uchar const *            payload,
                                  uint const *             txn_off,
                                  uint const *             txn_sz,
                                  ulong                    payload_sz,
                                  schar *                  txn_err,
                                  uint *                   sig_base,
                                  schar *                  sig_err );

/* The two calls above with the dedup tags (fd_ed25519_amd.h, "Dedup tags")
   as two more optional outputs, either may be NULL:
     txn_tag[t]  txn_cnt entries: the tag of transaction t's FIRST signature,
                 which is what the verify tile publishes for it
                 (fd_tango_amd.h); 0 for FD_TXN_AMD_ERR_PARSE.
     sig_tag[s]  one per signature slot, in the numbering of sig_err (so
                 sig_base is required with it, and the capacity is that of
                 sig_err); 0 in the slots of a payload that failed to parse.
   Both NULL is exactly the untagged call.  The multi-device form numbers
   sig_tag over the whole batch, as it does sig_err. */
int
fd_ed25519_amd_verify_txns_tag( fd_ed25519_amd_t * eng,
                                ulong              txn_cnt,
                                uchar const *      payload,
                                uint const *       txn_off,
                                uint const *       txn_sz,
                                ulong              payload_sz,
                                schar *            txn_err,
                                uint *             sig_base,
                                schar *            sig_err,
                                ulong *            txn_tag,
                                ulong *            sig_tag );

int
fd_ed25519_amd_multi_verify_txns_tag( fd_ed25519_amd_multi_t * multi,
                                      ulong                    txn_cnt,
                                      uchar const *            payload,
                                      uint const *             txn_off,
                                      uint const *             txn_sz,
                                      ulong                    payload_sz,
                                      schar *                  txn_err,
                                      uint *                   sig_base,
                                      schar *                  sig_err,
                                      ulong *                  txn_tag,
                                      ulong *                  sig_tag );

/* Transaction batch from registered memory: fd_ed25519_amd_verify_txns
   [_tag] in pointer-array form and without its staging.  txn[t] and a ulong
   txn_sz[t] replace payload, txn_off, txn_sz and payload_sz; every output
   is exactly that of fd_ed25519_amd_verify_txns[_tag] for the same payloads:
   the same txn_err codes (FD_TXN_AMD_ERR_PARSE included), the same global
   sig_base numbering (fd_ed25519_amd_txn_slots_ptrs), the same sig_err,
   txn_tag and sig_tag, with the engine's verdict mode applied.  The
   untagged function is the tagged one with both tag pointers NULL.

   The host copies no payload byte.  Per chunk it writes one 32-B record per
   transaction (a device address, the size, an offset, the signature-slot
   base) and a kernel (k_gather_txn) fetches the payloads over PCIe into the
   device blob that the GPU parser and the verify kernels read, and writes
   the chunk's offset, size and slot planes itself: a chunk needs no
   host-to-device copy.  Chunks are cut by fd_ed25519_amd_txn_gather_layout
   and go through every engine slot (FD_ED25519_AMD_NSLOT).

   Requirement: every non-empty [txn[t], +txn_sz[t]) lies inside ONE
   registration made through fd_ed25519_amd_host_register (its first and its
   last byte in the same one; two adjacent registrations do not make one
   range; only that table is consulted, as for
   fd_ed25519_amd_verify_batch_registered).  Payloads may have any byte
   alignment, may repeat and may overlap.  txn[t] is not looked at when
   txn_sz[t] is 0; such a payload gets FD_TXN_AMD_ERR_PARSE.

   Every transaction is checked before anything launches: a NULL array, a
   NULL txn[t] with txn_sz[t] > 0, txn_sz[t] > FD_TXN_AMD_MTU or > blob_max,
   a payload that reserves more than batch_max signature slots, sig_err or
   sig_tag given without sig_base, or a range the table does not hold
   returns FD_ED25519_AMD_ERR_INVAL with every output untouched and nothing
   in flight.  Addresses are translated again per chunk; the GPU is never
   given an address the table did not produce.

   Memory that changes during the call is the caller's error, but the result
   fails closed: the host reserves payload[0] signature slots from a byte it
   read before the GPU fetched the payload, and the GPU parser rejects
   (FD_TXN_AMD_ERR_PARSE) a transaction whose parsed signature count differs
   from its reserved slots and writes only inside them, so no signature is
   verified in, and no verdict is written to, a slot the host did not
   reserve for that transaction. */
int
fd_ed25519_amd_verify_txns_registered( fd_ed25519_amd_t *   eng,
                                       ulong                txn_cnt,
                                       void const * const * txn,
                                       ulong const *        txn_sz,
                                       schar *              txn_err,
                                       uint *               sig_base,
                                       schar *              sig_err );

int
fd_ed25519_amd_verify_txns_registered_tag( fd_ed25519_amd_t *   eng,
                                           ulong                txn_cnt,
                                           void const * const * txn,
                                           ulong const *        txn_sz,
                                           schar *              txn_err,
                                           uint *               sig_base,
                                           schar *              sig_err,
                                           ulong *              txn_tag,
                                           ulong *              sig_tag );

/* ===== Packed descriptors =====

   The fd_txn_t of every transaction that parses, laid end to end with an
   offset table, from the GPU parser -- so that what sits behind a verify
   tile (dedup, pack, the bank) need not run fd_txn_parse again on the CPU.

   Layout, the same in all three calls below:
     desc_off[0] = 0, desc_off[t+1] = desc_off[t] + footprint[t], txn_cnt+1
     entries, where footprint[t] is what fd_txn_parse returns for payload t
     (0 for a payload it rejects).  Footprints are even, so every offset is
     even; there is no padding between descriptors, and the running sum is
     carried in 64 bits.
     The descriptor of an accepted transaction t is the footprint[t] bytes at
     desc + desc_off[t], byte-identical to what fd_txn_parse writes.  A
     rejected payload occupies no bytes and no byte is written for it.

   Out of scope: the multi-device forms (a shard's base depends on the other
   shards' totals), the streaming tile (its 1408-B output frames have no room
   for a 3570-B descriptor), the drop-in call, and, in the synchronous calls
   and the plain submissions, filtering descriptors by verdict (the _keep
   submissions below pack descriptors for the survivors only). */

/* Upper bound on fd_txn_parse's footprint for ANY payload of payload_sz
   bytes (pure host code): 0 below 134 bytes, the smallest payload that
   parses (1 + 64 + 3 + 1 + 32 + 32 + 1), and above FD_TXN_AMD_PAYLOAD_MAX;
   otherwise 20 + 10*((payload_sz - 134)/3), capped at FD_TXN_MAX_SZ up to
   FD_TXN_AMD_MTU.  Every instruction takes at least 3 payload bytes for its
   10 descriptor bytes and every lookup table at least 34 for its 8, so with
   i instructions and l tables 3 i + 34 l <= payload_sz - 134 and the
   footprint 20 + 10 i + 8 l <= 20 + 10 (i + 11 l) <= the bound.  It is
   reached: 355 empty instructions at the MTU have footprint 3570. */
ulong
fd_txn_amd_desc_bound( ulong payload_sz );

/* Device-resident packed parse: fd_txn_amd_parse_dev's inputs (payloads up
   to 65535 B are accepted, as there); d_footprint[txn_cnt] as there;
   d_desc_off[txn_cnt+1] (8-aligned) and d_desc (2-aligned) in the layout
   above.  Capacity: descriptor t is stored only if d_desc_off[t+1] <=
   desc_cap, otherwise nothing of it is; no byte at or beyond d_desc +
   desc_cap is ever written (d_desc may be NULL when desc_cap is 0);
   d_desc_off is complete either way, so d_desc_off[txn_cnt] > desc_cap tells
   the caller that the tail is missing.  d_scratch: at least
   fd_txn_amd_parse_packed_scratch_footprint( txn_cnt ) bytes of device
   memory, 8-aligned, contents irrelevant.  Enqueued on `stream` without a
   sync; txn_cnt == 0 writes d_desc_off[0] only.

   A validate-only parse gives the footprints, an exclusive scan the offsets,
   and a second walk of the accepted payloads stores each descriptor at its
   offset (the parser stores records while it walks, before it knows that
   the payload is acceptable, so the first walk cannot have the final
   destination).  The scan is kernels ordered by the stream -- per-block
   totals, one workgroup that loops over them, a per-block pass -- and no
   workgroup ever waits for another. */
int
fd_txn_amd_parse_packed_dev( ulong         txn_cnt,
                             uchar const * d_payload,
                             uint const *  d_txn_off,
                             uint const *  d_txn_sz,
                             uint *        d_footprint,
                             ulong *       d_desc_off,
                             uchar *       d_desc,
                             ulong         desc_cap,
                             void *        d_scratch,
                             void *        stream );

ulong
fd_txn_amd_parse_packed_scratch_footprint( ulong txn_cnt );

/* fd_ed25519_amd_verify_txns_tag / fd_ed25519_amd_verify_txns_registered_tag
   that also return the packed descriptors.  desc_off (txn_cnt+1 entries) and
   desc (desc_cap bytes) are plain caller memory, numbered over the whole
   batch in the layout above; every other output is exactly that of the _tag
   call for the same arguments, in the engine's verdict mode.  A descriptor
   is returned for every transaction that parses, whatever its signatures'
   verdicts (descriptors do not depend on the mode):
   desc_off[t+1] == desc_off[t] exactly where txn_err[t] ==
   FD_TXN_AMD_ERR_PARSE, the registered call's fail-closed rejection of a
   payload whose parsed signature count differs from its reserved slots
   included.

   desc_off == NULL (then desc must be NULL too) is exactly the _tag call:
   nothing more is allocated, launched or copied; the _tag functions are
   these with NULL.

   Checked with the other arguments, before anything launches and with every
   output left untouched: desc given without desc_off or desc_off without
   desc, and desc_cap smaller than the sum of fd_txn_amd_desc_bound(
   txn_sz[t] ) over the batch, return FD_ED25519_AMD_ERR_INVAL.  Capacity is
   decided by the bound and never by the data, so a batch that passes cannot
   overflow.  On an error return the contents of desc and desc_off are
   unspecified, as for the verdicts and tags.

   Per chunk the descriptors are packed in device memory and one kernel
   copies the chunk's offsets and bytes to the slot's mapped host staging,
   reading the byte total on the device; the host adds the running byte base
   when it drains the slot, chunks in the order they were launched.  The
   staging (per slot at most min( 3570*batch_max, 20*batch_max +
   10*blob_max/3 ) bytes, device and pinned host) is allocated by the first
   call that asks for descriptors. */
int
fd_ed25519_amd_verify_txns_desc( fd_ed25519_amd_t * eng,
                                 ulong              txn_cnt,
                                 uchar const *      payload,
                                 uint const *       txn_off,
                                 uint const *       txn_sz,
                                 ulong              payload_sz,
                                 schar *            txn_err,
                                 uint *             sig_base,
                                 schar *            sig_err,
                                 ulong *            txn_tag,
                                 ulong *            sig_tag,
                                 ulong *            desc_off,
                                 uchar *            desc,
                                 ulong              desc_cap );

int
fd_ed25519_amd_verify_txns_registered_desc( fd_ed25519_amd_t *   eng,
                                            ulong                txn_cnt,
                                            void const * const * txn,
                                            ulong const *        txn_sz,
                                            schar *              txn_err,
                                            uint *               sig_base,
                                            schar *              sig_err,
                                            ulong *              txn_tag,
                                            ulong *              sig_tag,
                                            ulong *              desc_off,
                                            uchar *              desc,
                                            ulong                desc_cap );

/* Asynchronous submissions of the two calls above: one chunk on one slot,
   launched now and delivered later by fd_ed25519_amd_async_poll /
   fd_ed25519_amd_async_wait.  The contract is "Asynchronous submissions" in
   fd_ed25519_amd.h; what is particular to transactions:
   - one chunk: the staged form's transactions number at most batch_max,
     their signature slots (fd_ed25519_amd_txn_slots) total at most batch_max
     and their bytes at most blob_max; for the registered form
     fd_ed25519_amd_txn_gather_layout over the whole submission returns
     txn_cnt.  Otherwise, and for txn_cnt == 0, FD_ED25519_AMD_ERR_INVAL;
   - sig_base (when given) is written by the submit call, every other output
     at delivery; txn_tag, sig_tag, sig_err, desc_off / desc are optional as
     in the synchronous calls;
   - desc_off is relative to the submission (desc_off[0] == 0) and desc_cap
     is checked against the submission's bound sum;
   - the staged form copies the payload bytes during submit; the registered
     form's payloads are read until delivery. */
int
fd_ed25519_amd_submit_txns( fd_ed25519_amd_t * eng,
                            ulong              txn_cnt,
                            uchar const *      payload,
                            uint const *       txn_off,
                            uint const *       txn_sz,
                            ulong              payload_sz,
                            schar *            txn_err,
                            uint *             sig_base,
                            schar *            sig_err,
                            ulong *            txn_tag,
                            ulong *            sig_tag,
                            ulong *            desc_off,
                            uchar *            desc,
                            ulong              desc_cap,
                            ulong *            ticket );

int
fd_ed25519_amd_submit_txns_registered( fd_ed25519_amd_t *   eng,
                                       ulong                txn_cnt,
                                       void const * const * txn,
                                       ulong const *        txn_sz,
                                       schar *              txn_err,
                                       uint *               sig_base,
                                       schar *              sig_err,
                                       ulong *              txn_tag,
                                       ulong *              sig_tag,
                                       ulong *              desc_off,
                                       uchar *              desc,
                                       ulong                desc_cap,
                                       ulong *              ticket );

/* The two submissions above that also return the publish list: "Survivors"
   in fd_ed25519_amd.h, with transactions as the items -- transaction t is a
   survivor iff txn_err[t] == 0 and ( its tag, the tag of its first
   signature, is 0 or no earlier passing transaction of the submission has
   it ).  keep (capacity txn_cnt) and keep_cnt come before ticket; both NULL
   is exactly the submit call above, one without the other
   FD_ED25519_AMD_ERR_INVAL.  Written at delivery: keep[0, keep_cnt), the
   survivors' indices ascending, and *keep_cnt; nothing at or beyond
   keep[keep_cnt].
   - The tags the filter needs are gathered into a device plane whether or
     not txn_tag was asked for.  txn_err, txn_tag, sig_tag, sig_err and
     sig_base stay what the submit call above delivers, for all transactions.
   - Descriptors, when asked for, are packed for the survivors only: desc_off
     keeps its txn_cnt + 1 entries and its layout, and desc_off[t+1] ==
     desc_off[t] exactly where t is not a survivor; a survivor's bytes are
     those the unfiltered call returns for it.  The pack runs behind the
     filter on the footprints it masked.  desc_cap is still checked against
     the submission's bound sum.
   Out of scope, as there: the synchronous calls, the multi-device engine, the
   tile, dedup across submissions. */
int
fd_ed25519_amd_submit_txns_keep( fd_ed25519_amd_t * eng,
                                 ulong              txn_cnt,
                                 uchar const *      payload,
                                 uint const *       txn_off,
                                 uint const *       txn_sz,
                                 ulong              payload_sz,
                                 schar *            txn_err,
                                 uint *             sig_base,
                                 schar *            sig_err,
                                 ulong *            txn_tag,
                                 ulong *            sig_tag,
                                 ulong *            desc_off,
                                 uchar *            desc,
                                 ulong              desc_cap,
                                 uint *             keep,
                                 ulong *            keep_cnt,
                                 ulong *            ticket );

int
fd_ed25519_amd_submit_txns_registered_keep( fd_ed25519_amd_t *   eng,
                                            ulong                txn_cnt,
                                            void const * const * txn,
                                            ulong const *        txn_sz,
                                            schar *              txn_err,
                                            uint *               sig_base,
                                            schar *              sig_err,
                                            ulong *              txn_tag,
                                            ulong *              sig_tag,
                                            ulong *              desc_off,
                                            uchar *              desc,
                                            ulong                desc_cap,
                                            uint *               keep,
                                            ulong *              keep_cnt,
                                            ulong *              ticket );

/* Output frames of the transaction family ("Output frames" in
   fd_ed25519_amd.h, which states the rule): survivor j's frame is payload
   (P) | zeros up to round_up( P, 16 ) | fd_txn_t (F) | P as a little-endian
   u16, at out + emit_off[j], emit_sz[j] = round_up( P, 16 ) + F + 2 bytes.
   - fd_txn_amd_emit_bound( payload_sz ): 0 where fd_txn_amd_desc_bound is 0,
     otherwise round_up( round_up( payload_sz, 16 ) + fd_txn_amd_desc_bound(
     payload_sz ) + 2, 128 ): at least the stride of any frame of a payload
     of that size (met with equality by the MTU payload of 355 empty
     instructions).  Pure host code.
   - fd_txn_amd_emit: the rule on the host, over pointer arrays; desc_off /
     desc as the _desc calls return them (F = desc_off[i+1] - desc_off[i]).
     Returns the total; out == NULL only computes the layout; a total above
     out_cap returns ~0UL and writes nothing.
   - fd_txn_amd_emit_dev: the step alone, device-resident, with
     fd_ed25519_amd_emit_dev's conventions, capacity rule and bounds.  The
     inputs are the payload planes and what fd_txn_amd_parse_packed_dev left
     (d_desc_off: txn_cnt + 1 entries, 8-aligned; d_desc).  A payload above
     FD_TXN_AMD_PAYLOAD_MAX bytes has a frame of size 0; a payload the parser
     rejected has F = 0.
   - The _emit submissions: the _keep forms above with out, out_cap, emit_off
     and emit_sz in front of ticket, under the rules stated there (the bound
     is fd_txn_amd_emit_bound).  The frames are read from the slot's device
     copy of the payloads and from the descriptors packed on the masked
     footprints: the pack runs when emit is asked for even with desc == NULL;
     desc / desc_off stay independent optional outputs. */
ulong
fd_txn_amd_emit_bound( ulong payload_sz );

ulong
fd_txn_amd_emit( ulong                keep_cnt,
                 uint const *         keep,
                 void const * const * txn,
                 ulong const *        txn_sz,
                 ulong const *        desc_off,
                 uchar const *        desc,
                 void *               out,
                 ulong                out_cap,
                 ulong *              emit_off,
                 uint *               emit_sz );

int
fd_txn_amd_emit_dev( ulong         txn_cnt,
                     uchar const * d_payload,
                     uint const *  d_txn_off,
                     uint const *  d_txn_sz,
                     ulong const * d_desc_off,
                     uchar const * d_desc,
                     uint const *  d_keep,
                     ulong const * d_keep_cnt,
                     void *        d_out,
                     ulong         out_cap,
                     ulong *       d_emit_off,
                     uint *        d_emit_sz,
                     void *        d_scratch,
                     void *        stream );

int
fd_ed25519_amd_submit_txns_emit( fd_ed25519_amd_t * eng,
                                 ulong              txn_cnt,
                                 uchar const *      payload,
                                 uint const *       txn_off,
                                 uint const *       txn_sz,
                                 ulong              payload_sz,
                                 schar *            txn_err,
                                 uint *             sig_base,
                                 schar *            sig_err,
                                 ulong *            txn_tag,
                                 ulong *            sig_tag,
                                 ulong *            desc_off,
                                 uchar *            desc,
                                 ulong              desc_cap,
                                 uint *             keep,
                                 ulong *            keep_cnt,
                                 void *             out,
                                 ulong              out_cap,
                                 ulong *            emit_off,
                                 uint *             emit_sz,
                                 ulong *            ticket );

int
fd_ed25519_amd_submit_txns_registered_emit( fd_ed25519_amd_t *   eng,
                                            ulong                txn_cnt,
                                            void const * const * txn,
                                            ulong const *        txn_sz,
                                            schar *              txn_err,
                                            uint *               sig_base,
                                            schar *              sig_err,
                                            ulong *              txn_tag,
                                            ulong *              sig_tag,
                                            ulong *              desc_off,
                                            uchar *              desc,
                                            ulong                desc_cap,
                                            uint *               keep,
                                            ulong *              keep_cnt,
                                            void *               out,
                                            ulong                out_cap,
                                            ulong *              emit_off,
                                            uint *               emit_sz,
                                            ulong *              ticket );

/* ===== Compute budget =====

   Per transaction, the two numbers pack (or any scheduler) needs first: how
   many compute units it may burn and what it pays on top of the signature
   fee -- what the reference's fd_compute_budget_program_init / _parse /
   _finalize (src/ballet/pack/fd_compute_budget_program.h:71-204) make of the
   instructions addressed to ComputeBudget111111111111111111111111111111 --
   from the GPU, which holds the payload already, so that the consumer need
   not walk every instruction's program address and data again.

   The record of transaction t, payload p of sz bytes, descriptor d as
   fd_txn_parse writes it.  24 bytes, 8-aligned, little endian:
     rewards       *out_rewards of fd_compute_budget_program_finalize
     compute       *out_compute
     heap_sz       the state's heap_size
     flags         the state's flags, FD_TXN_AMD_BUDGET_FLAG_* (the
                   reference's bit values; it #undefs its own macros)
     cb_instr_cnt  the state's compute_budget_instr_cnt
     status        FD_TXN_AMD_BUDGET_OK, _INVALID or _NOPARSE

   _NOPARSE iff the transaction has no descriptor: footprint 0, or wherever
   the calling entry point reports FD_TXN_AMD_ERR_PARSE (the registered
   calls' fail-closed rejection included).  Every other field is 0.

   Otherwise instr[0 .. instr_cnt) are walked in order from a zeroed state.
   Instruction i is a compute-budget instruction iff instr[i].program_id <
   acct_addr_cnt and the 32 bytes at p + acct_addr_off + 32*program_id equal
   the id.  The bound on program_id is ours, and deliberate: fd_txn_parse
   (fd_txn_parse.c:200) lets program_id reach into the lookup-table accounts,
   whose addresses are not in the payload, and comparing whatever bytes follow
   the address array (with program_id == acct_addr_cnt, the recent blockhash)
   would let those bytes pose as the program.  Such an instruction is never a
   compute-budget instruction here.  Each match runs
   fd_compute_budget_program_parse on p[data_off, +data_sz), exactly: data_sz
   < 5 is rejected before the discriminant is looked at; then the per-kind
   sizes (9, 5, 5, 9 for discriminants 0 to 3, no other discriminant), the
   duplicate rules (RequestUnitsDeprecated counts as both a limit and a
   price) and the 1024 granularity of the heap.

   _INVALID: the first instruction it rejects ends the walk, and every other
   field is 0 (the reference has written heap_size by the time the
   granularity check fails; that partial state does not leak).

   _OK otherwise, with fd_compute_budget_program_finalize( state, instr_cnt ):
   without a limit set, cu_limit = (instr_cnt - cb_instr_cnt) * 200000 as a
   64-bit value; compute is its low 32 bits and the fee arithmetic uses all
   64 (they differ from 21475 non-budget instructions up, which only payloads
   above the MTU reach).  With FLAG_SET_TOTAL_FEE rewards is total_fee,
   otherwise min( 2^64 - 1, ceil( cu_limit * micro_lamports_per_cu / 10^6 ) ),
   computed in the reference's split form without 128-bit arithmetic.

   Verdicts, the verdict mode, keep and the window play no part: a record is
   defined for every transaction, as a descriptor is, and a caller that
   publishes keep[j] reads budget[keep[j]].  Whether an _INVALID transaction
   is forwarded stays the caller's decision.

   - fd_txn_amd_budget: the rule on the host, over one payload and its
     descriptor (txn == NULL: _NOPARSE).  Makes no device call.  The
     descriptor is trusted as fd_txn_parse's for this payload, but an address
     or a data range of it that ends beyond payload_sz gives _NOPARSE rather
     than a read outside the payload.  Returns the status.
   - fd_txn_amd_budget_dev: the step alone, device-resident, with the
     conventions of the other _dev calls: the caller's stream, no sync,
     payloads up to 65535 B as fd_txn_amd_parse_dev takes them.  The inputs
     are the payload planes and the footprint plane fd_txn_amd_parse_dev left
     (0: _NOPARSE).  One lane per transaction walks the payload under a
     checked cursor: no contents of the inputs cause a read outside
     [d_payload + d_txn_off[t], + d_txn_sz[t]), and a bound that fails -- it
     cannot after a genuine parse -- ends in _NOPARSE.  d_budget: 8-aligned
     device or mapped host memory, prior contents irrelevant; d_budget[t] is
     written for every t < txn_cnt and nothing else is.  txn_cnt == 0
     launches nothing.
   - The four engine calls: fd_ed25519_amd_verify_txns_desc, its registered
     form and the two _emit submissions, each with fd_txn_amd_budget_t *
     budget (capacity txn_cnt, plain caller memory), in front of ticket where
     there is one.  budget == NULL is exactly the call it extends: nothing
     more is allocated, launched or copied, and the existing functions are
     these with NULL.  Otherwise one more kernel goes on the slot's stream
     right behind k_txn_parse -- ahead of the verify kernels, outside the
     stretch a dedup window serialises among submissions -- and writes the
     chunk's records into the slot's budget plane (24 * batch_max bytes of
     mapped pinned memory, allocated by the first call that asks); they reach
     budget the way txn_tag does: per chunk in the blocking calls, at
     delivery by the reporting fd_ed25519_amd_async_poll / _wait in the
     submissions, for all txn_cnt transactions, survivors or not.  Every rule
     of "Asynchronous submissions" holds: error returns, BUSY and an
     undelivered submission leave budget untouched.  Every other output is
     byte for byte that of the same call without budget.
   Out of scope, as for descriptors: the multi-device forms, the streaming
   tile, the drop-in call, and any change to the emit frame. */
#define FD_TXN_AMD_BUDGET_OK      (0U)
#define FD_TXN_AMD_BUDGET_INVALID (1U)
#define FD_TXN_AMD_BUDGET_NOPARSE (2U)

#define FD_TXN_AMD_BUDGET_FLAG_SET_CU        ((ushort)0x01)   /* fd_compute_budget_program.h:29-32 */
#define FD_TXN_AMD_BUDGET_FLAG_SET_FEE       ((ushort)0x02)
#define FD_TXN_AMD_BUDGET_FLAG_SET_HEAP      ((ushort)0x04)
#define FD_TXN_AMD_BUDGET_FLAG_SET_TOTAL_FEE ((ushort)0x08)

struct fd_txn_amd_budget {
  ulong  rewards;
  uint   compute;
  uint   heap_sz;
  ushort flags;
  ushort cb_instr_cnt;
  uint   status;
};
typedef struct fd_txn_amd_budget fd_txn_amd_budget_t;

int
fd_txn_amd_budget( uchar const *         payload,
                   ulong                 payload_sz,
                   fd_txn_t const *      txn,
                   fd_txn_amd_budget_t * out );

int
fd_txn_amd_budget_dev( ulong                 txn_cnt,
                       uchar const *         d_payload,
                       uint const *          d_txn_off,
                       uint const *          d_txn_sz,
                       uint const *          d_footprint,
                       fd_txn_amd_budget_t * d_budget,
                       void *                stream );

int
fd_ed25519_amd_verify_txns_budget( fd_ed25519_amd_t *    eng,
                                   ulong                 txn_cnt,
                                   uchar const *         payload,
                                   uint const *          txn_off,
                                   uint const *          txn_sz,
                                   ulong                 payload_sz,
                                   schar *               txn_err,
                                   uint *                sig_base,
                                   schar *               sig_err,
                                   ulong *               txn_tag,
                                   ulong *               sig_tag,
                                   ulong *               desc_off,
                                   uchar *               desc,
                                   ulong                 desc_cap,
                                   fd_txn_amd_budget_t * budget );

int
fd_ed25519_amd_verify_txns_registered_budget( fd_ed25519_amd_t *    eng,
                                              ulong                 txn_cnt,
                                              void const * const *  txn,
                                              ulong const *         txn_sz,
                                              schar *               txn_err,
                                              uint *                sig_base,
                                              schar *               sig_err,
                                              ulong *               txn_tag,
                                              ulong *               sig_tag,
                                              ulong *               desc_off,
                                              uchar *               desc,
                                              ulong                 desc_cap,
                                              fd_txn_amd_budget_t * budget );

int
fd_ed25519_amd_submit_txns_budget( fd_ed25519_amd_t *    eng,
                                   ulong                 txn_cnt,
                                   uchar const *         payload,
                                   uint const *          txn_off,
                                   uint const *          txn_sz,
                                   ulong                 payload_sz,
                                   schar *               txn_err,
                                   uint *                sig_base,
                                   schar *               sig_err,
                                   ulong *               txn_tag,
                                   ulong *               sig_tag,
                                   ulong *               desc_off,
                                   uchar *               desc,
                                   ulong                 desc_cap,
                                   uint *                keep,
                                   ulong *               keep_cnt,
                                   void *                out,
                                   ulong                 out_cap,
                                   ulong *               emit_off,
                                   uint *                emit_sz,
                                   fd_txn_amd_budget_t * budget,
                                   ulong *               ticket );

int
fd_ed25519_amd_submit_txns_registered_budget( fd_ed25519_amd_t *    eng,
                                              ulong                 txn_cnt,
                                              void const * const *  txn,
                                              ulong const *         txn_sz,
                                              schar *               txn_err,
                                              uint *                sig_base,
                                              schar *               sig_err,
                                              ulong *               txn_tag,
                                              ulong *               sig_tag,
                                              ulong *               desc_off,
                                              uchar *               desc,
                                              ulong                 desc_cap,
                                              uint *                keep,
                                              ulong *               keep_cnt,
                                              void *                out,
                                              ulong                 out_cap,
                                              ulong *               emit_off,
                                              uint *                emit_sz,
                                              fd_txn_amd_budget_t * budget,
                                              ulong *               ticket );

/* Signature-slot numbering of a pointer-array batch (pure host code, no
   device): the rule of fd_ed25519_amd_txn_slots, one payload per pointer.
   txn[t] is not looked at when txn_sz[t] is 0, and a NULL txn[t] reserves
   no slot.  tbase has txn_cnt+1 entries; returns the total. */
ulong
fd_ed25519_amd_txn_slots_ptrs( ulong                txn_cnt,
                               void const * const * txn,
                               ulong const *        txn_sz,
                               uint *               tbase );

/* How fd_ed25519_amd_verify_txns_registered cuts a batch into chunks (pure
   host code, no device): of n payloads with sizes sz[] and signature-slot
   counts slots[], one chunk takes the first -- always -- and further ones
   while the count stays <= cap, the slot total stays <= cap (the engine's
   batch_max bounds both) and the padded byte total, the sum of
   round_up( sz[i], 16 ), stays <= blob_cap (its blob_max).  Returns the
   number taken and writes dst[0 .. that), each payload's offset in the
   chunk's device blob (a multiple of 16, ascending), and *slot_cnt, the
   chunk's signature slots. */
ulong
fd_ed25519_amd_txn_gather_layout( ulong         n,
                                  ulong const * sz,
                                  uint const *  slots,
                                  ulong         cap,
                                  ulong         blob_cap,
                                  uint *        dst,
                                  ulong *       slot_cnt );

/* Device-resident form (inputs already in HBM, caller's stream, no sync).
   Signature slots follow the same rule as fd_ed25519_amd_verify_txns:
   d_tbase[t] (txn_cnt+1 entries, slot_cnt = d_tbase[txn_cnt]) is what
   fd_ed25519_amd_txn_slots computes on the host.  d_sig_err (optional,
   slot_cnt entries) receives the per-signature codes.  d_ws: at least
   fd_ed25519_amd_txn_workspace_footprint(txn_cnt, slot_cnt) bytes,
   256-aligned; it begins with the signature verify's workspace, so
   fd_ed25519_amd_work_stats_dev( slot_cnt, d_ws, ... ) reads the call's
   per-signature work statistics.

   Contract on memory, as for fd_ed25519_amd_verify_dev: d_ws may hold
   anything on entry -- for instance the slots of an earlier batch, each
   with a signature that verified -- and no result depends on it: the parse
   kernel marks or fills every slot of [0, slot_cnt) (d_tbase must cover
   them: d_tbase[0] = 0, ascending), and a slot of a payload that did not
   parse is never verified, whatever it holds.  The call writes
   d_ws[0, footprint), d_txn_err[0, txn_cnt), d_sig_err[0, slot_cnt) --
   every entry -- and nothing else; d_payload, d_txn_off, d_txn_sz and
   d_tbase are only read. */
ulong
fd_ed25519_amd_txn_workspace_footprint( ulong txn_cnt, ulong slot_cnt );

ulong
fd_ed25519_amd_txn_slots( ulong         txn_cnt,
                          uchar const * payload,
                          uint const *  txn_off,
                          uint const *  txn_sz,
                          uint *        tbase );

int
fd_ed25519_amd_verify_txns_dev( ulong         txn_cnt,
                                ulong         slot_cnt,
                                uchar const * d_payload,
                                uint const *  d_txn_off,
                                uint const *  d_txn_sz,
                                uint const *  d_tbase,
                                schar *       d_txn_err,
                                schar *       d_sig_err,
                                void *        d_ws,
                                void *        stream );

/* Verdict mode of the transaction entry points (fd_ed25519_amd.h,
   FD_ED25519_AMD_MODE_*).  fd_ed25519_amd_verify_txns and the multi-device
   form follow their engine's mode (fd_ed25519_amd_set_mode /
   fd_ed25519_amd_multi_set_mode); the device-resident form takes it as an
   argument.  In FD_ED25519_AMD_MODE_STRICT every signature gets the strict
   verdict and the transaction rule is unchanged: the first failing
   signature's code, so a transaction with an s-window signature or a
   torsion-point signer is rejected (-1 / -2).  FD_TXN_AMD_ERR_PARSE is the
   same in both modes.  Any other mode: FD_ED25519_AMD_ERR_INVAL, checked
   first. */
int
fd_ed25519_amd_verify_txns_dev_mode( ulong         txn_cnt,
                                     ulong         slot_cnt,
                                     uchar const * d_payload,
                                     uint const *  d_txn_off,
                                     uint const *  d_txn_sz,
                                     uint const *  d_tbase,
                                     schar *       d_txn_err,
                                     schar *       d_sig_err,
                                     void *        d_ws,
                                     void *        stream,
                                     int           mode );

/* Per-transaction dedup tags of the last fd_ed25519_amd_verify_txns_dev*
   call on workspace d_ws, with the d_tbase it was given (txn_cnt+1 entries):
   d_txn_tag[t] = the tag of transaction t's first signature, 0 for a
   transaction that did not parse (txn_cnt entries, device or mapped host
   memory, 8-aligned).  The per-signature tags of the same call are
   fd_ed25519_amd_tags_dev( slot_cnt, d_ws, ... ).  Enqueued on `stream`,
   no sync. */
int
fd_ed25519_amd_txn_tags_dev( ulong        txn_cnt,
                             uint const * d_tbase,
                             void const * d_ws,
                             ulong *      d_txn_tag,
                             void *       stream );

/* Workload synthesis (config 4): txn_cnt well-formed legacy / v0
   transactions with nsig_lo..nsig_hi signers (account addresses = the
   next public keys of pub[]) and ~msg_lo..msg_hi-byte messages, capped at
   the MTU; signature fields zero.  Per signature: its message range in
   payload (sig_msg_off, sig_msg_sz) and where its 64 bytes go (sig_at).
   Returns the signature count, 0 if payload_cap / pub_cnt is too small. */
ulong
fd_ed25519_amd_synth_txns( ulong         seed,
                           ulong         txn_cnt,
                           uint          nsig_lo,
                           uint          nsig_hi,
                           uint          msg_lo,
                           uint          msg_hi,
                           uchar const * pub,
                           ulong         pub_cnt,
                           uchar *       payload,
                           ulong         payload_cap,
                           uint *        txn_off,
                           uint *        txn_sz,
                           uint *        sig_msg_off,
                           uint *        sig_msg_sz,
                           uint *        sig_at );

#ifdef __cplusplus
}
#endif

#endif /* HEADER_fd_txn_amd_h */
