/*
 * rsync_hip.h -- C-ABI of librsynchip.so: java-rsync's delta-transfer checksum path on MI355X (gfx950).
 *
 * The reference (alpapad/java-rsync, Java 8) has no native/FFI seam; the seam this library fills is
 * the two private hot methods and their helpers (paths relative to
 * core/src/main/java/com/github/java/rsync/internal/):
 *
 *   Generator.sendItemizeAndChecksums  session/Generator.java:866-909  -> rsh_block_sums[_device]
 *   Sender.sendMatchesAndData          session/Sender.java:1235-1327   -> rsh_match_scan[_device]
 *   Sender.skipMatchSendData           session/Sender.java:1386-1399   -> rsh_match_scan (block_length 0)
 *   Generator.getBlockLengthFor        session/Generator.java:198-206  -> rsh_block_length_for
 *   Generator.getDigestLength          session/Generator.java:208-212  -> rsh_digest_length_for
 *   Checksum.Header(int,int,long)      session/Checksum.java:94-113    -> rsh_header_make
 *   Checksum.Header(int,int,int,int)   session/Checksum.java:75-92     -> rsh_header_validate
 *   Sender.sendDataFrom + putInt(...)  session/Sender.java:794-809,1274,1316,1148 -> rsh_tokens_write
 *
 * A JNI shim (java-rsync_amd/jni/) binds these for the Java side; see INTEGRATION.md.
 * Plain pointers and sizes only; the caller owns every host buffer.  One rsh_ctx per calling thread
 * (the reference runs Generator and Sender on separate threads, RsyncClient.java:431); contexts are
 * independent and may target different devices (file-parallel sharding).
 */
#ifndef RSYNC_HIP_H
#define RSYNC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSH_ABI_VERSION 5

/* Status codes (the JNI shim maps them onto the reference's exception types). */
#define RSH_OK 0
#define RSH_E_INVAL (-1)    /* bad argument (IllegalArgumentException)                      */
#define RSH_E_PROTOCOL (-2) /* header fails Checksum.Header 4-arg validation (RsyncProtocolException,
                               Connection.java:28-38)                                        */
#define RSH_E_OVERFLOW (-3) /* chunk count > Integer.MAX_VALUE (Checksum.ChunkOverflow, :107-111) */
#define RSH_E_NOSPACE (-4)  /* event buffer too small; *n_ev holds the count needed          */
#define RSH_E_DEVICE (-5)   /* HIP runtime / kernel failure, or no gfx950 device present     */
#define RSH_E_NOMEM (-6)    /* host or device allocation failed                              */
#define RSH_E_BUSY (-7)     /* the context is serving a call on another thread               */
#define RSH_E_NOTFOUND (-8) /* the file does not exist (FileViewNotFound, FileView.java:74-75)    */
#define RSH_E_OPEN (-9)     /* the file cannot be opened (FileViewOpenFailed, FileView.java:76-78) */
#define RSH_E_NOSOURCE (-10) /* the context holds no source from its last scan (tiled, trimmed, or reused since) */

/* Checksum.Header; wire order of Connection.sendChecksumHeader (Connection.java:40-45) is
 * chunk_count, block_length, digest_length, remainder (4 x little-endian int32).
 * Any 0 < block_length <= 131072 is legal (Checksum.java:75-92) and gives the same results; block lengths from 512 up
 * run on the coalesced kernels, multiples of 128 or not ("Block lengths a peer may send"). */
typedef struct {
    int32_t chunk_count;
    int32_t block_length;
    int32_t digest_length;
    int32_t remainder;
} rsh_header;

/* One Sender action.  RSH_EV_LITERAL = one sendDataFrom(buf, offset, length) call (length > 0; the
 * 8 KiB token split happens at replay, Sender.java:794-809).  RSH_EV_MATCH = `count` consecutive
 * putInt(-(i+1)) for chunks index .. index+count-1, matched at consecutive windows starting at file
 * offset `offset`; `length` = the bytes those windows add to sizeMatch (Sender.java:1269). */
enum { RSH_EV_LITERAL = 1, RSH_EV_MATCH = 2 };
typedef struct {
    int64_t offset;
    int64_t length;
    int32_t kind;
    int32_t index;
    int32_t count;
    int32_t reserved;
} rsh_event;

/* Per-scan counters (diagnostics; not part of the reference's output). */
typedef struct {
    int64_t chain_matches;   /* matches resolved by the aligned speculation fast path          */
    int64_t events;          /* candidate events the resolver evaluated                       */
    int64_t probe_launches;  /* range-probe kernel launches                                   */
    int64_t host_md5_windows;/* single-window digests computed on the host (resolver misses)  */
    int64_t flushes;         /* FileView.isFull flushes (Sender.java:1294-1302)                */
    double device_ms;        /* wall time of the bulk device phase (speculation kernels + copies) */
    double resolver_ms;      /* host resolver time (including its small device round trips)   */
    double table_ms;         /* host index of the received table (chained hash, built lazily)  */
    int64_t head_steps;      /* resolver steps taken before the aligned speculation landed    */
    int64_t speculation_aborted; /* 1: the scan ended first and the speculation launch was stopped;
                                    2: the scan ended in head mode before the speculation was launched;
                                    3: a tentative launch was stopped at once (the lead windows differ) */
    int64_t device_bytes;    /* source bytes the device work of this scan read: speculations that ran to
                                completion (a stopped one counts 0), probed ranges (+ B - 1 per interval),
                                weak-sum windows, gathered bytes and copied digest windows (ABI 2)  */
    int64_t phase_launches;  /* phase-shifted speculations launched (chains at kB + delta, ABI 2)   */
    int64_t phase_matches;   /* matches resolved from a phase-shifted speculation (ABI 2)           */
    double spec_kernel_ms;   /* the aligned speculation's K1 alone (HIP events on its stream), when it ran
                                to completion; 0 otherwise (ABI 2)                                   */
    double phase_kernel_ms;  /* the phase-shifted speculations' K1s that ran to completion, summed (ABI 2) */
    int64_t phase_guesses;   /* phase-shifted speculations started before the resolver, at the phase found
                                past a sampled run's end (ABI 2)                                     */
} rsh_scan_stats;

typedef struct rsh_ctx rsh_ctx;

int rsh_abi_version(void);
const char* rsh_strerror(int status);
/* Text of the calling thread's last HIP failure (error string and source line), "" if none. */
const char* rsh_last_error(void);
int rsh_device_count(int* count);
int rsh_ctx_create(int device, rsh_ctx** out);
void rsh_ctx_destroy(rsh_ctx* ctx);
/* hipStream_t the context launches on (opaque), for callers composing with their own streams. */
void* rsh_ctx_stream(rsh_ctx* ctx);

/* ---- sizing / header (pure host functions) ---- */
int32_t rsh_block_length_for(int64_t file_size);                                    /* Generator.java:198-206 */
int32_t rsh_digest_length_for(int64_t file_size, int32_t block_length, int32_t min_digest_length); /* :208-212,:873 */
int rsh_header_make(int32_t block_length, int32_t digest_length, int64_t file_size, rsh_header* out);
int rsh_header_validate(const rsh_header* h);

/* ---- Generator: per-chunk weak + MD5(chunk || seed)[0:digest_length] (Generator.java:886-895) ----
 * weak_out[chunk_count]; strong_out[chunk_count * digest_length].  Host buffers. */
int rsh_block_sums(rsh_ctx* ctx, const uint8_t* data, int64_t n, const rsh_header* h, const uint8_t seed[4],
                   int32_t* weak_out, uint8_t* strong_out);
/* Device-resident form: d_data, d_weak, d_strong are device pointers; runs on the context stream and
 * returns after the work is enqueued (rsh_ctx_sync waits). */
int rsh_block_sums_device(rsh_ctx* ctx, const void* d_data, int64_t n, const rsh_header* h, const uint8_t seed[4],
                          void* d_weak, void* d_strong);
int rsh_ctx_sync(rsh_ctx* ctx);
/* Releases the context's pass-sized buffers -- the segment passes' HBM (rsh_*_batch: up to 2 x the segment_bytes
 * budget, 16 GiB by default), the Receiver passes' and the host-input staging -- after waiting for the context's
 * streams.  The next call that needs them allocates them again.  The batched scan's state (chunk index, hit map,
 * descriptors, pinned event buffers: bounded by the largest segment's chunks and option chain_map_bytes) stays, so
 * that the next segment scan costs what the previous one did.  A JVM holding
 * several contexts on one GPU (a local transfer's Generator and Sender) calls it after each segment; see
 * INTEGRATION.md "Per-context memory".  Replaces nothing in the reference (its buffers are Java heap). */
int rsh_ctx_trim(rsh_ctx* ctx);

/* ---- Sender (Sender.java:1098-1148 per-file glue, :1235-1327 scan, :1386-1399 new file) ----
 * h: the header received from the Generator (validated here exactly as Connection.receiveChecksumHeader
 * does); weak[chunk_count], strong[chunk_count * digest_length]: the received table.
 * Events are written to ev[0..ev_cap); *n_ev receives the count (RSH_E_NOSPACE if ev_cap is short).
 * file_md5 = MD5 of the whole source (Sender.java:1241,1326); literal/matched = sizeLiteral/sizeMatch. */
int rsh_match_scan(rsh_ctx* ctx, const uint8_t* src, int64_t n, const rsh_header* h, const int32_t* weak,
                   const uint8_t* strong, const uint8_t seed[4], rsh_event* ev, int64_t ev_cap, int64_t* n_ev,
                   uint8_t file_md5[16], int64_t* literal, int64_t* matched, rsh_scan_stats* stats);
/* Device-resident form: source and table already in HBM (d_src, d_weak, d_strong).  The serial
 * whole-file MD5 is not computed here (see rsh_file_md5); everything else is identical. */
int rsh_match_scan_device(rsh_ctx* ctx, const void* d_src, int64_t n, const rsh_header* h, const void* d_weak,
                          const void* d_strong, const uint8_t seed[4], rsh_event* ev, int64_t ev_cap,
                          int64_t* n_ev, int64_t* literal, int64_t* matched, rsh_scan_stats* stats);

/* Tiled form for sources larger than the device (BASELINE config 3; FileView streams any file through a
 * 10*B window, FileView.java:235-278): the source stays in host memory and HBM holds one tile of tile_bytes
 * (rounded to a multiple of B, at least 16*B; 0 = 4 GiB) plus a 16*B halo at a time, paged in as the scan
 * advances; the aligned speculation runs tile by tile.  Events, literal and matched are those of
 * rsh_match_scan.  file_md5 may be NULL (the serial whole-file digest is then skipped). */
int rsh_match_scan_tiled(rsh_ctx* ctx, const uint8_t* src, int64_t n, const rsh_header* h, const int32_t* weak,
                         const uint8_t* strong, const uint8_t seed[4], int64_t tile_bytes, rsh_event* ev,
                         int64_t ev_cap, int64_t* n_ev, uint8_t file_md5[16], int64_t* literal, int64_t* matched,
                         rsh_scan_stats* stats);

/* After RSH_E_NOSPACE from rsh_match_scan[_device] the context keeps that scan's events: fetch them into
 * a buffer of at least *n_ev entries without recomputing (valid until the context's next scan). */
int rsh_fetch_events(rsh_ctx* ctx, rsh_event* ev, int64_t ev_cap, int64_t* n_ev);

/* Whole-file MD5 on the host (one serial chain; runs beside the device work). */
int rsh_file_md5(const uint8_t* data, int64_t n, uint8_t out[16]);

/* ---- channel bytes ----
 * Exact bytes Sender writes for one file: per literal event the 8 KiB-split putInt(len)+bytes tokens,
 * per matched chunk putInt(-(index+1)), then putInt(0) and the 16-byte file MD5. */
int64_t rsh_tokens_size(const rsh_event* ev, int64_t n_ev);
int rsh_tokens_write(const uint8_t* src, const rsh_event* ev, int64_t n_ev, const uint8_t file_md5[16],
                     uint8_t* out, int64_t cap);
/* ---- channel bytes from a source in HBM ----
 * The same bytes framed on the device (token_frame_kernel) when the source the scan read is in HBM: no second pass
 * over the file, and the literal bytes sent are the ones that were scanned and digested, as in the reference, which
 * sends them out of the FileView buffer it scanned (Sender.java:794-809).  These forms write bytes [from, from + len)
 * of the stream rsh_tokens_write would produce into the host buffer `out` (any memory; the library stages through its
 * own pinned buffers), so that a caller pulls a stream larger than one buffer window by window.  Every event is
 * checked on the host before anything is launched: RSH_E_INVAL for a literal with offset < 0, length <= 0 or
 * offset + length > n, for a match with count <= 0, index < 0 or index + count above int32, for an unknown kind, and
 * for from < 0, len < 0 or from + len > rsh_tokens_size.  len == 0 launches nothing; a stream without literals needs
 * no source. */
int rsh_tokens_write_device(rsh_ctx* ctx, const void* d_src, int64_t n, const rsh_event* ev, int64_t n_ev,
                            const uint8_t file_md5[16], int64_t from, uint8_t* out, int64_t len);
/* The same bytes, after the same checks, into device memory [d_out, d_out + len) at any byte alignment, trailer
 * included: the kernel writes straight to d_out (no staging, no host copy), so that a Receiver on the same device
 * takes the stream where it lies (rsh_receiver_combine_resident). */
int rsh_tokens_frame_device(rsh_ctx* ctx, const void* d_src, int64_t n, const rsh_event* ev, int64_t n_ev,
                            const uint8_t file_md5[16], int64_t from, void* d_out, int64_t len);
/* The same over the source the context's last single-file scan left in HBM: rsh_match_scan (block_length > 0),
 * rsh_match_scan_file below option file_tile_above (a new file included) and rsh_match_scan_pieces when resident
 * record it; every other call that uses the context's buffers, rsh_ctx_trim and a failed scan drop it (the lifetime of
 * the events rsh_fetch_events returns).  RSH_E_NOSOURCE when there is none: the caller then replays the literals
 * from its own copy of the file. */
int rsh_tokens_write_kept(rsh_ctx* ctx, const rsh_event* ev, int64_t n_ev, const uint8_t file_md5[16], int64_t from,
                          uint8_t* out, int64_t len);
/* A segment: every file's whole stream, one job per file, device sources, host outputs; the spans of all files share
 * the launches.  Per job: RSH_E_NOSPACE with out_len = the size needed when out_cap is short, RSH_E_INVAL for that
 * file's bad events; the other files are still written.  Returns RSH_OK or the first failing job's status. */
typedef struct {
    const void* d_src;
    int64_t n;
    const rsh_event* ev;   /* host */
    int64_t n_ev;
    uint8_t file_md5[16];
    uint8_t* out;          /* host, caller-owned: out_cap bytes */
    int64_t out_cap;
    int64_t out_len;       /* out: the stream's size */
    int32_t status;        /* out */
    int32_t reserved;
} rsh_token_job;
int rsh_tokens_write_batch_device(rsh_ctx* ctx, rsh_token_job* jobs, int32_t njobs);
/* The same segment into device memory: every file's whole stream, trailer included, at d_out (any byte alignment), so
 * that a segment's Receiver on the same device takes the streams where they lie
 * (rsh_receiver_combine_batch_resident).  The checks and per-job statuses are those of the form above; the spans of
 * all files point straight at their d_out and run in one launch, and the trailers of all files are placed by one more. */
typedef struct {
    const void* d_src;
    int64_t n;
    const rsh_event* ev;   /* host */
    int64_t n_ev;
    uint8_t file_md5[16];
    void* d_out;           /* device, caller-owned: out_cap bytes */
    int64_t out_cap;
    int64_t out_len;       /* out: the stream's size */
    int32_t status;        /* out */
    int32_t reserved;
} rsh_token_frame_job;
int rsh_tokens_frame_batch_device(rsh_ctx* ctx, rsh_token_frame_job* jobs, int32_t njobs);

/* Generator channel bytes: header + per chunk putInt(weak) + digest_length bytes. */
int64_t rsh_generator_bytes(const rsh_header* h, const int32_t* weak, const uint8_t* strong, uint8_t* out,
                            int64_t cap);

/* ---- batched files (one segment of the file list) ----
 * The reference handles a segment's files one after another: the Generator sends every file's header +
 * table (Generator.java:558-614, sendItemizeAndChecksums :866-909 per file) and the Sender answers each in
 * turn (Sender.sendFiles :1098-1148 -> sendMatchesAndData :1235-1327).  The batched forms take all the
 * files of a segment at once, so their kernels fill the device: one K1 launch for every file's block
 * sums, and one resolver per file whose device round trips are gathered into one launch per round.
 * Results are per file and identical to the single-file calls.  All pointers in a job are device
 * pointers except ev (host).  Returns RSH_OK, or the first failing job's status (every job's own status
 * is in its `status`). */
typedef struct {
    const void* d_data;  /* the basis file */
    int64_t n;
    rsh_header h;        /* as for rsh_block_sums (3-arg Checksum.Header semantics) */
    void* d_weak;        /* out: chunk_count weak sums */
    void* d_strong;      /* out: chunk_count * digest_length digest bytes */
} rsh_block_job;
int rsh_block_sums_batch_device(rsh_ctx* ctx, const rsh_block_job* jobs, int32_t njobs, const uint8_t seed[4]);

typedef struct {
    const void* d_src;     /* the source file */
    int64_t n;
    rsh_header h;          /* the received header (validated as by rsh_match_scan) */
    const void* d_weak;    /* the received table */
    const void* d_strong;
    rsh_event* ev;         /* host, caller-owned: ev_cap entries */
    int64_t ev_cap;
    int64_t n_ev;          /* out: event count (RSH_E_NOSPACE in status if > ev_cap; events then lost) */
    int64_t literal;       /* out */
    int64_t matched;       /* out */
    int32_t status;        /* out: RSH_OK or an error code for this file */
    int32_t reserved;
} rsh_scan_job;
/* stats (optional): summed over the files (device_ms / resolver_ms: wall time of the whole batch). */
int rsh_match_scan_batch_device(rsh_ctx* ctx, rsh_scan_job* jobs, int32_t njobs, const uint8_t seed[4],
                                rsh_scan_stats* stats);

/* ---- file ingest: the FileView reads of the two passes (FileView.java:51-80 open, :187-278 reads) ----
 * The file is read straight into pinned staging buffers by several threads (large preads), copied to the
 * device piece by piece while the next piece is read, and summed there.  `size` is the size the caller's
 * FileInfo holds (FileView reads exactly that many bytes): a file that ends early or fails to read is
 * zero-filled from that point, the result is computed over those bytes, and *read_error is set -- the
 * reference's deferred FileViewException at close() (the Sender then flips md5[0], Sender.java:1136-1143).
 * size == 0 opens nothing (FileView.java:62-72).
 * rsh_block_sums_file: the Generator pass; the device holds two pieces at a time, so the file may be
 * larger than HBM.  rsh_match_scan_file: the Sender pass; the source is assembled in HBM while a host
 * thread digests the pieces in order (the whole-file MD5 of Sender.java:1241,1326). */
int rsh_block_sums_file(rsh_ctx* ctx, const char* path, int64_t size, const rsh_header* h, const uint8_t seed[4],
                        int32_t* weak_out, uint8_t* strong_out, int32_t* read_error);
int rsh_match_scan_file(rsh_ctx* ctx, const char* path, int64_t size, const rsh_header* h, const int32_t* weak,
                        const uint8_t* strong, const uint8_t seed[4], rsh_event* ev, int64_t ev_cap, int64_t* n_ev,
                        uint8_t file_md5[16], int64_t* literal, int64_t* matched, rsh_scan_stats* stats,
                        int32_t* read_error);

/* ---- a file handed over as a list of host buffers ----
 * A JVM cannot hold a file above 2^31 - 1 bytes in one direct ByteBuffer, while the reference streams any
 * file size through FileView (FileView.java:51-80,235-278).  These forms take the file as pieces (each a
 * caller-owned host buffer; the file is their concatenation, in order; a chunk or window may straddle
 * two pieces) and return exactly what rsh_block_sums / rsh_match_scan return for the concatenated bytes.
 * The Sender's literal events name file offsets; the binding replays each from the pieces
 * (INTEGRATION.md).  Sources above 32 GiB are paged through HBM a tile at a time. */
typedef struct {
    const uint8_t* data;
    int64_t len;
} rsh_piece;
int rsh_block_sums_pieces(rsh_ctx* ctx, const rsh_piece* pieces, int32_t npieces, const rsh_header* h,
                          const uint8_t seed[4], int32_t* weak_out, uint8_t* strong_out);
int rsh_match_scan_pieces(rsh_ctx* ctx, const rsh_piece* pieces, int32_t npieces, const rsh_header* h,
                          const int32_t* weak, const uint8_t* strong, const uint8_t seed[4], rsh_event* ev,
                          int64_t ev_cap, int64_t* n_ev, uint8_t file_md5[16], int64_t* literal, int64_t* matched,
                          rsh_scan_stats* stats);

/* ---- a segment's files from host memory (ABI 4) ----
 * What a Java Generator / Sender holding a file-list segment in JVM buffers calls: Generator.itemizeSegment
 * (Generator.java:558-614) sends every file's header + table (sendItemizeAndChecksums :866-909 per file), and
 * Sender.sendFiles (Sender.java:1098-1148) answers each file in turn with sendMatchesAndData (:1235-1327), whose
 * last 16 bytes are the whole-file MD5 (:1241,1326).  These forms take the whole segment in one call: each file
 * is a list of caller-owned host pieces (as rsh_*_pieces), the bytes are copied to HBM (up to a budget of about
 * 16 GiB per pass; a file larger than that goes through the tiled single-file path), every file's sums or scan
 * run in the batched device forms above, and -- for the Sender -- every file's MD5 runs on the host's cores
 * beside the copies and the scan, several files per core (rsh_file_md5_batch).  Per-file results equal the
 * single-file calls'.  Returns RSH_OK, or the first failing job's status; every job's own status is in it
 * (RSH_E_NOSPACE: ev_cap was short, n_ev holds the count needed and the file's events are not kept). */
typedef struct {
    const rsh_piece* pieces; /* the basis file: the concatenation of its pieces (npieces 0: an empty file) */
    int32_t npieces;
    int32_t status;          /* out */
    rsh_header h;            /* 3-arg Checksum.Header of the file (as for rsh_block_sums) */
    int32_t* weak_out;       /* host: chunk_count weak sums */
    uint8_t* strong_out;     /* host: chunk_count * digest_length digest bytes */
} rsh_block_batch_job;
int rsh_block_sums_batch(rsh_ctx* ctx, rsh_block_batch_job* jobs, int32_t njobs, const uint8_t seed[4]);

typedef struct {
    const rsh_piece* pieces; /* the source file */
    int32_t npieces;
    int32_t status;          /* out */
    rsh_header h;            /* the received header (validated as by rsh_match_scan) */
    const int32_t* weak;     /* host: the received table */
    const uint8_t* strong;
    rsh_event* ev;           /* host, caller-owned: ev_cap entries */
    int64_t ev_cap;
    int64_t n_ev;            /* out */
    int64_t literal;         /* out: sizeLiteral */
    int64_t matched;         /* out: sizeMatch */
    uint8_t file_md5[16];    /* out: MD5 of the whole source (Sender.java:1241,1326) */
} rsh_scan_batch_job;
/* stats (optional): summed over the files, as rsh_match_scan_batch_device's. */
int rsh_match_scan_batch(rsh_ctx* ctx, rsh_scan_batch_job* jobs, int32_t njobs, const uint8_t seed[4],
                         rsh_scan_stats* stats);

/* ---- the checksum table in wire form ----
 * The bytes the Generator writes for one file and the Sender reads: the 16 header bytes of
 * Connection.sendChecksumHeader (Connection.java:40-45), then chunk_count records of 4 + digest_length bytes, the
 * little-endian weak sum and the digest bytes (Generator.java:888-895; read back by Sender.receiveChecksumsFor,
 * Sender.java:758-767).  rsh_generator_bytes above is the definition.  The device forms convert between these bytes
 * and the two arrays in HBM that the block sums write and the scans read (sums_frame_kernel / sums_unframe_kernel), for
 * every digest_length >= 0 (a peer may send more than the Generator's 16). */
/* 16 + chunk_count * (4 + digest_length); RSH_E_INVAL for a negative count or length.  Pure host. */
int64_t rsh_sums_wire_size(const rsh_header* h);
/* Connection.receiveChecksumHeader (Connection.java:28-38): the four ints parsed, then the 4-arg validation:
 * RSH_E_PROTOCOL exactly where rsh_header_validate gives it (*out is then untouched).  Pure host. */
int rsh_header_from_wire(const uint8_t wire[16], rsh_header* out);
/* Header + table of the sums in HBM (d_weak, d_strong) into the host buffer `out` (any memory; staged through the
 * library's pinned buffer).  h is the Generator's own header (any block length its 3-arg constructor makes);
 * RSH_E_INVAL for a negative count or length, RSH_E_NOSPACE when cap is short of rsh_sums_wire_size. */
int rsh_sums_frame_device(rsh_ctx* ctx, const rsh_header* h, const void* d_weak, const void* d_strong, uint8_t* out,
                          int64_t cap);
/* The records as received (host memory, no header; len must equal chunk_count * (4 + digest_length), else
 * RSH_E_INVAL) into d_weak and d_strong, which rsh_match_scan_device and rsh_match_scan_batch_device then take. */
int rsh_sums_unframe_device(rsh_ctx* ctx, const rsh_header* h, const uint8_t* records, int64_t len, void* d_weak,
                            void* d_strong);

/* ---- a segment's files from host memory, in channel bytes ----
 * The two segment calls above with the reference's channel bytes on both sides, so that the Java side moves each
 * file's table and reply with one bulk put / get instead of a loop per chunk or per token.
 * Generator: `out` receives header + table exactly as Generator.sendItemizeAndChecksums writes them (a pass's tables
 * are framed by one kernel launch; an empty file's 16 header bytes and the table of a file larger than a pass come
 * from the host).  Per-file statuses as rsh_block_sums_batch, plus RSH_E_NOSPACE (out_len = the size needed) for a
 * short out_cap, which fails that file only. */
typedef struct {
    const rsh_piece* pieces; /* the basis file */
    int32_t npieces;
    int32_t status;          /* out */
    rsh_header h;            /* as rsh_block_batch_job */
    uint8_t* out;            /* host, caller-owned: out_cap bytes */
    int64_t out_cap;
    int64_t out_len;         /* out: rsh_sums_wire_size(&h) */
} rsh_block_wire_job;
int rsh_block_sums_batch_wire(rsh_ctx* ctx, rsh_block_wire_job* jobs, int32_t njobs, const uint8_t seed[4]);
/* Sender: one transfer request and its whole reply.  `table` holds the file's records as they came off the channel
 * (after the header, which the caller parsed with rsh_header_from_wire); they go to HBM raw and are unframed there.
 * status, ev, n_ev, literal, matched and file_md5 are rsh_match_scan_batch's (a short ev_cap is RSH_E_NOSPACE in
 * status, and then there is no stream; table_len other than chunk_count * (4 + digest_length) is RSH_E_INVAL for that
 * file only).  `out` receives the bytes of rsh_tokens_write: each pass's streams are framed from the sources the pass
 * holds in HBM, before the next pass replaces them; a new file (block_length 0) and an empty source are framed from
 * the pieces.  out_status: RSH_OK when the stream is in `out`; RSH_E_NOSPACE (out_len = the size needed) when out_cap
 * is short; RSH_E_NOSOURCE for a file larger than a pass, scanned tiled; the status's code when the scan failed.  With
 * NOSPACE and NOSOURCE the events are valid and the caller replays them itself.
 * A caller that must flip md5[0] after a read error (Sender.java:1136-1143) overwrites the last 16 bytes of `out`. */
typedef struct {
    const rsh_piece* pieces; /* the source file */
    int32_t npieces;
    int32_t status;          /* out */
    rsh_header h;            /* the received header (validated as by rsh_match_scan) */
    const uint8_t* table;    /* host: the received records */
    int64_t table_len;
    rsh_event* ev;           /* host, caller-owned: ev_cap entries */
    int64_t ev_cap;
    int64_t n_ev;            /* out */
    int64_t literal;         /* out */
    int64_t matched;         /* out */
    uint8_t file_md5[16];    /* out */
    uint8_t* out;            /* host, caller-owned: out_cap bytes */
    int64_t out_cap;
    int64_t out_len;         /* out: the stream's size */
    int32_t out_status;      /* out */
    int32_t reserved;
} rsh_send_job;
int rsh_match_scan_batch_wire(rsh_ctx* ctx, rsh_send_job* jobs, int32_t njobs, const uint8_t seed[4],
                              rsh_scan_stats* stats);

/* Whole-file MD5s of many files (pure host; no context): md5[16] of each job = MD5 of its pieces'
 * concatenation.  Independent files run side by side, up to 16 per core (AVX-512; 8 with AVX2), on `threads`
 * threads (0 = the process's cores, cgroup quota included). */
typedef struct {
    const rsh_piece* pieces;
    int32_t npieces;
    int32_t reserved;
    uint8_t md5[16];         /* out */
} rsh_md5_job;
int rsh_file_md5_batch(rsh_md5_job* jobs, int32_t njobs, int32_t threads);

/* ---- whole-file MD5s of files in HBM (Sender.java:1241,1326; Receiver.java:824-842) ----
 * What the *_device entry points leave to the caller, for files that stay in HBM: md5[16] of each job = MD5 of the n
 * device bytes at d_data.  It is for MANY files: one file's MD5 is a serial chain, so each file runs on one lane of
 * file_md5_kernel (64 files to a wave, longest first; DESIGN.md section 4, "Whole-file MD5s on the device") at about a
 * tenth of a host core's rate (75 MB/s per file), and a segment's files run side by side.  A single file, or a few, are
 * digested faster by downloading the bytes for rsh_file_md5_batch.  Measured on one MI355X against the download and
 * the host's 16 cores: at files of 64 KiB this call wins from 64 files on, the fewest measured
 * (0.90 against 1.13 ms), at files of 1 MiB from about 330 files on (14.0 ms whatever the count up to 8192, against
 * 6.3 ms at 128 files and 38.5 ms at 1024).  A launch advances a file by at most option md5_device_slice bytes; longer
 * files take several launches.
 * Synchronous.  Per job: RSH_E_INVAL for n < 0, or n > 0 with a null d_data; the other files are still digested.
 * Returns RSH_OK or the first failing job's status in file order (RSH_E_INVAL for a null ctx, or null jobs with
 * njobs > 0).  njobs == 0 and a segment of empty files launch nothing; an empty file's digest is d41d8cd9...427e. */
typedef struct {
    const void* d_data;   /* device; any byte alignment */
    int64_t n;
    uint8_t md5[16];      /* out */
    int32_t status;       /* out */
    int32_t reserved;
} rsh_md5_device_job;     /* 40 bytes */
int rsh_file_md5_batch_device(rsh_ctx* ctx, rsh_md5_device_job* jobs, int32_t njobs);

/* ---- Receiver (Receiver.java:459-555 combineDataToFile, :557-578 copies, :204-209 blockSize) ----
 * Replays one file's de-multiplexed token stream -- putInt(len)+bytes, putInt(-(i+1)), putInt(0), exactly
 * what rsh_tokens_write produces -- against the replica (the basis the Generator summed; NULL when the
 * Receiver has none: matches are then skipped, :487-494).  The target receives the literal bytes and the
 * replica blocks in token order; with defer_write (and a replica) nothing is written while the matches
 * are 0, 1, 2, ... in order with no literal, and a stream that matched all chunk_count blocks that way
 * leaves the file intact (out->intact = 1, the replica is the result, :529-545).  out->md5 is the digest
 * the Receiver computes over the file content; compare it with the 16 bytes that follow the stream
 * (isRemoteAndLocalFileIdentical, :824-842).  Status: RSH_E_PROTOCOL for a block index out of range or a
 * match against block_length 0 (RsyncProtocolException, :480-485); RSH_E_INVAL for a truncated stream
 * or a replica shorter than a block it names (IllegalStateException, :1012-1017); RSH_E_NOSPACE when
 * target_cap < out->target_len (nothing written). */
typedef struct {
    int64_t tokens_used;  /* bytes consumed, including the terminating putInt(0) */
    int64_t target_len;   /* bytes of the rebuilt file written to the target (0 when intact) */
    int64_t literal;      /* sizeLiteral */
    int64_t matched;      /* sizeMatch */
    int32_t intact;       /* combineDataToFile's return value */
    int32_t reserved;
    uint8_t md5[16];
} rsh_combine_result;
/* Host buffers (the replica is uploaded, the target downloaded). */
int rsh_receiver_combine(rsh_ctx* ctx, const uint8_t* tokens, int64_t tokens_len, const rsh_header* h,
                         const uint8_t* replica, int64_t replica_len, int32_t defer_write, uint8_t* target,
                         int64_t target_cap, rsh_combine_result* out);
/* Device-resident replica and target (the tokens stay in host memory); the blocks are gathered by a
 * kernel, the literal bytes uploaded in one copy; the digest is computed on the host from the result. */
int rsh_receiver_combine_device(rsh_ctx* ctx, const uint8_t* tokens, int64_t tokens_len, const rsh_header* h,
                                const void* d_replica, int64_t replica_len, int32_t defer_write, void* d_target,
                                int64_t target_cap, rsh_combine_result* out);
/* The stream in device memory too (a local transfer: Sender, Generator and Receiver on one device): the token walk
 * runs on the device and only its run list comes down -- no stream byte crosses PCIe; literal runs are placed from
 * the raw stream by a kernel.  Results and statuses are those of the form above for the same bytes (of several errors
 * the first offending token in stream order decides).  flags: 0, or RSH_COMBINE_NO_MD5. */
#define RSH_COMBINE_NO_MD5 1   /* out->md5 zeroed: the caller digests the bytes it downloads anyway */
int rsh_receiver_combine_resident(rsh_ctx* ctx, const void* d_tokens, int64_t tokens_len, const rsh_header* h,
                                  const void* d_replica, int64_t replica_len, int32_t defer_write, void* d_target,
                                  int64_t target_cap, int32_t flags, rsh_combine_result* out);
/* A segment of such files in one call: one job per file, every pointer a device pointer.  Each job gets exactly what
 * rsh_receiver_combine_resident gives for the same arguments -- result, status, target bytes; a failed file's target
 * is untouched.  The files' walks share launches (token_scan_batch_kernel, a workgroup per file; a file whose run list
 * of option tokens_runs_batch records was full walks on in the next round), every file's ranges are one gather launch
 * and every file's literal runs one unframe launch.  Unless flags has RSH_COMBINE_NO_MD5 the result bytes then come
 * to the host, as many files at a time as option resident_md5_bytes of pinned staging holds, and are digested side by
 * side on the host's cores.  Returns RSH_OK or the first failing job's status in file order; a call that fails as a
 * whole (RSH_E_DEVICE) leaves every file it did not finish with its code.  njobs == 0 launches nothing. */
typedef struct {
    const void* d_tokens;     /* the file's token stream, ending with putInt(0) */
    int64_t tokens_len;
    rsh_header h;
    const void* d_replica;    /* NULL: none */
    int64_t replica_len;
    int32_t defer_write;
    int32_t status;           /* out */
    void* d_target;           /* target_cap bytes (nothing written when intact) */
    int64_t target_cap;
    rsh_combine_result res;   /* out */
} rsh_resident_job;
int rsh_receiver_combine_batch_resident(rsh_ctx* ctx, rsh_resident_job* jobs, int32_t njobs, int32_t flags);

/* ---- a segment's Receiver from host memory (Receiver.receiveFiles, Receiver.java:1145-1263: combineDataToFile
 * :459-556 and isRemoteAndLocalFileIdentical :824-842 for each file in turn) ----
 * One job per file: its de-multiplexed token stream, its replica as host pieces (nreplica 0: no replica), the
 * target buffer.  Each job gets rsh_receiver_combine's result and its own status (RSH_E_PROTOCOL / RSH_E_INVAL /
 * RSH_E_NOSPACE as there); a call that fails as a whole leaves every file it did not finish with its code.  The
 * rebuilt files are gathered on the device (the token streams and the replica ranges they name go up, every file's
 * blocks and literals are one gather launch, the targets come back) in passes of at most option segment_bytes,
 * overlapped; the verify digests -- one serial MD5 chain per file -- run on the host's cores beside the copies,
 * up to 16 files per core (md5_mb.cpp), over the replica ranges and literal bytes the tokens name, which are
 * exactly the rebuilt file's bytes.  A file is never split across passes: one whose token stream, replica ranges and
 * target together exceed segment_bytes gets a pass of its own of that size, and fails with RSH_E_NOMEM when the
 * device cannot hold it (the single-file rsh_receiver_combine's limit: its target and replica in HBM at once). */
typedef struct {
    const uint8_t* tokens;    /* host: the file's token stream, ending with putInt(0) */
    int64_t tokens_len;
    rsh_header h;             /* the file's checksum header (as sent by the Generator) */
    const rsh_piece* replica; /* host: the replica as pieces (their concatenation); NULL / 0 pieces: none */
    int32_t nreplica;
    int32_t defer_write;
    uint8_t* target;          /* host, caller-owned: target_cap bytes (nothing written when intact) */
    int64_t target_cap;
    int32_t status;           /* out */
    int32_t reserved;
    rsh_combine_result res;   /* out */
} rsh_combine_job;
int rsh_receiver_combine_batch(rsh_ctx* ctx, rsh_combine_job* jobs, int32_t njobs);

/* ---- a segment over several GPUs (ABI 5) ----
 * north_star: "files shard embarrassingly across the 8 GPUs of one node".  In the reference one thread walks every
 * file of a transfer: the Generator sums a segment's files in turn (Generator.java:558-614,806-860), one Sender thread
 * answers each (Sender.sendFiles, Sender.java:978-1170) and one Receiver thread rebuilds each (Receiver.java:1145-1263).
 * These forms take the calling thread's contexts ctxs[0 .. nctx) -- distinct contexts, typically one per GPU of the
 * node (several on one GPU also work: they run side by side there) -- split the segment's files over them by
 * rsh_shard_files, and run each context's share as the single-context call above (rsh_block_sums_batch,
 * rsh_match_scan_batch, rsh_receiver_combine_batch) on a host thread of its own, the process's cores shared evenly
 * among those threads.  No data moves between GPUs.  Every job's outputs and status are exactly what the
 * single-context call gives that file; a failure on one context marks only the files that context had not finished.
 * Returns RSH_OK, or the first failing job's status in file order (RSH_E_INVAL for a null or repeated context).
 * stats: summed over the contexts.  nctx == 1 is the single-context call. */
int rsh_block_sums_batch_multi(rsh_ctx* const* ctxs, int32_t nctx, rsh_block_batch_job* jobs, int32_t njobs,
                               const uint8_t seed[4]);
int rsh_match_scan_batch_multi(rsh_ctx* const* ctxs, int32_t nctx, rsh_scan_batch_job* jobs, int32_t njobs,
                               const uint8_t seed[4], rsh_scan_stats* stats);
/* (the wire forms: the same split by the pieces' bytes) */
int rsh_block_sums_batch_wire_multi(rsh_ctx* const* ctxs, int32_t nctx, rsh_block_wire_job* jobs, int32_t njobs,
                                    const uint8_t seed[4]);
int rsh_match_scan_batch_wire_multi(rsh_ctx* const* ctxs, int32_t nctx, rsh_send_job* jobs, int32_t njobs,
                                    const uint8_t seed[4], rsh_scan_stats* stats);
/* (the Receiver's files are split by max(tokens_len, replica bytes): about the bytes each rebuilds) */
int rsh_receiver_combine_batch_multi(rsh_ctx* const* ctxs, int32_t nctx, rsh_combine_job* jobs, int32_t njobs);
/* The split (pure host): part_out[f] = the part (context) file f goes to.  Longest first by bytes (equal sizes in
 * file order), each file to the part with the fewest bytes so far (ties to the lower part): shard.py's rank rule. */
int rsh_shard_files(const int64_t* bytes, int32_t nfiles, int32_t nparts, int32_t* part_out);

/* ---- device buffers for the *_device entry points (callers without their own allocator, e.g. JNI) ---- */
int rsh_dev_alloc(rsh_ctx* ctx, int64_t bytes, void** out);
int rsh_dev_free(rsh_ctx* ctx, void* p);
int rsh_memcpy_h2d(rsh_ctx* ctx, void* dst, const void* src, int64_t bytes);  /* synchronous */
int rsh_memcpy_d2h(rsh_ctx* ctx, void* dst, const void* src, int64_t bytes);  /* synchronous */

/* ---- synthetic input for benchmarks: splitmix64 counter stream generated on the device ---- */
int rsh_fill_splitmix_device(rsh_ctx* ctx, void* d_out, int64_t n, uint64_t key, int64_t byte_offset);

#ifdef __cplusplus
}
#endif
#endif
