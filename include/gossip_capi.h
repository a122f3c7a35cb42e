/*
 * gossip_capi.h -- C-ABI of the MI355X gossip-propagation engine (libgossip_hip.so).
 *
 * The reference (Sidharthshanu/Gossip-protocol-with-power-law) has no FFI: its
 * hot path is one OS thread per TCP socket.  This ABI replaces, for ALL peers at
 * once, one round of
 *   - gossip generation + fan-out         Peer.py:395-408  (gossip_sender)
 *   - receive dispatch                    Peer.py:175-216, 258-296
 *   - forward-once / Message-List dedup   (spec-level: absent from the reference,
 *                                          SURVEY.md §0 finding 1)
 *   - heartbeat liveness + dead report    Peer.py:298-393, 128-151
 *   - seed dead-node removal              Seed.py:358-406
 * over an overlay built by the seed registry (Seed.py:127-149) or by the
 * degree-weighted selector (demonstrate_powerlaw.py:7-39).
 *
 * Conventions
 *   - Every function returns 0 on success and a negative gp_status on failure;
 *     gp_last_error() gives a thread-local message.  Nothing aborts or exits.
 *   - The caller owns host arrays; they are copied in.  The context owns all
 *     device memory.  One context = one device + one HIP stream; not thread-safe.
 *   - Vertex ids are 0..n-1 int32; arc offsets int64.  Messages are 0..m-1 and
 *     are packed 64 per uint64 word, W = ceil(m/64) rounded up to a power of two
 *     (1..64 words per vertex row, i.e. m <= 4096 per context; larger message
 *     sets are run as independent batches by the host -- messages never interact).
 *   - Multi-GPU: one process per GPU.  Either message shards (each context
 *     runs the whole overlay for a word-aligned block of messages,
 *     gp_config.msg_word_base; no collective), or a vertex partition
 *     (gp_set_partition, nranks > 1, undirected overlays): each context keeps
 *     its owned slice [vbegin, vend) plus ghost rows for the non-owned
 *     in-neighbours of owned vertices, and after every round sends each peer
 *     only the new bits of the boundary vertices that received something
 *     (ncclSend / ncclRecv over xGMI, gp_comm_init; or device-to-device copies
 *     in gp_round_group).  Per-vertex reads of a partitioned context return its
 *     owned slice; its CSR reads return the local CSR (GP_L2G maps local ids).
 */
#ifndef GOSSIP_CAPI_H
#define GOSSIP_CAPI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GP_ABI_VERSION 18

typedef struct gp_ctx gp_ctx;

typedef enum gp_status {
  GP_OK = 0,
  GP_EINVAL = -1,     /* bad argument / shape                              */
  GP_EHIP = -2,       /* HIP runtime error                                 */
  GP_ENOMEM = -3,     /* device allocation failed                          */
  GP_ESTATE = -4,     /* call out of order (e.g. round before load_graph)  */
  GP_ERCCL = -5,      /* RCCL error                                        */
  GP_ENOTRACK = -6    /* requested output was not tracked (see gp_config)  */
} gp_status;

/* Per-round counters (all exact integers, summed over ranks). */
typedef struct gp_round_stats {
  int32_t round;            /* r                                                      */
  int32_t overflow;         /* 1 if the report buffer overflowed this round          */
  uint64_t injected;        /* messages injected at live origins in round r          */
  uint64_t lost;            /* messages whose origin was down at their inject round  */
  uint64_t new_bits;        /* first receipts produced by round r (receipt round r+1)*/
  uint64_t receivers;       /* vertices with >= 1 first receipt in round r           */
  uint64_t sends;           /* edge-deliveries attempted in round r:
                               sum_u deg_live(u) * |frontier_r(u)|                   */
  uint64_t active;          /* senders with a non-empty frontier in round r          */
  uint64_t crashed;         /* vertices that crashed in round r                      */
  uint64_t reports;         /* "Dead Node" reports emitted in round r (Peer.py:311)  */
  uint64_t removals;        /* vertices removed by the seed (Seed.py:387-391)        */
  uint64_t dup_reports;     /* reports hitting "not found" (Seed.py:373-375)         */
  uint64_t arcs_scanned;    /* in-arcs visited by the pull (byte accounting)         */
  uint64_t rows_gathered;   /* neighbour Message-List rows loaded (8*W bytes each)   */
  uint64_t seen_rows_read;  /* receiver seen rows read (8*W bytes each)              */
  uint64_t rows_written;    /* receiver seen rows written to the next slot (8*W B)   */
  uint64_t vertices_visited;/* receivers whose in-list was scanned                   */
  uint64_t atomics;         /* push mode: 64-bit atomicOr issued                      */
  uint64_t next_arcs;       /* out-degree sum of this round's receivers (direction)   */
  uint64_t row_bytes;       /* bytes of neighbour rows actually loaded (the pull skips
                               the words a receiver already completed, §3.4)         */
  int32_t mode;             /* 0 = pull expansion, 1 = push expansion, 2 = expansion
                               over lossy or delayed links (gp_link_loss, gp_link_delay
                               below; scan is 0)                                      */
  int32_t scan;             /* pull arc check (bits 0-1 as a number): 0 = activity-
                               bitmap probe per arc, 1 = per-arc activity mask built
                               first, 2 = none, every in-neighbour row read (§3.4),
                               3 = probe, low-degree in-lists prefiltered (§3.2);
                               + 4: senders gathered from compact Message-Lists;
                               + 8: 64-word line masks read (only named 128-B lines
                               gathered, §3.2); + 16: those masks were written by
                               the previous round's commits (no k_mklm pass);
                               + 32: degree-split round (senders of in-degree <
                               split_deg pushed, receivers probe the gather-order
                               prefix of the others, §3.2); + 64: every scanned
                               arc probed the done bitmap (complete receivers
                               alias their component row, `aliased`, §3.2);
                               + 128: the waves took their receivers from the
                               list the previous round left (§3.5)                */
  double expand_ms;         /* device time of the expansion kernels (HIP events)     */
  double exchange_ms;       /* device time of the RCCL exchange (0 on 1 GPU)         */
  double round_ms;          /* device time of the whole round                        */
  double kernel_ms;         /* device time of the pull kernel + its hub passes (and
                               of a degree-split round's push half and clear)    */
  uint64_t xchg_rows;       /* vertex partition: boundary entries sent (all peers)   */
  uint64_t xchg_bytes;      /* vertex partition: bytes sent (entry heads + words)    */
  uint64_t done_nb;         /* receivers that took every message of their component
                               from an in-neighbour holding all of them (§3.4)      */
  uint64_t lm_rows;         /* senders' rows read to build line masks before a
                               filtered 64-word pull (8*W bytes each, §3.2)         */
  uint64_t aliased;         /* receivers that completed their component and took it
                               as their Message-List without writing a row (their
                               slot byte names the component row, §3.2; ABI 18)    */
} gp_round_stats;

/* One dead-node report: reporter saw `dead` miss 3 heartbeats in `round`. */
typedef struct gp_report {
  int32_t dead;
  int32_t reporter;
  int32_t round;
} gp_report;

typedef struct gp_config {
  int32_t track_first;         /* keep the u8 first-receipt matrix [n][m] (255 = never) */
  int32_t track_digest;        /* keep per-vertex first-receipt digest u64[n]          */
  int32_t track_msg_forwards;  /* accumulate per-message forwards every round          */
  int32_t churn;               /* run the liveness phase every round                   */
  double p_fail;               /* per-round crash probability of a live vertex         */
  uint64_t churn_seed;         /* crash draws: splitmix stream        */
  int32_t miss_threshold;      /* heartbeat misses before report (reference: 3)        */
  int32_t hub_threshold;       /* in-degree above which a vertex is split over waves   */
  int64_t report_capacity;     /* reports kept per round (counts stay exact)           */
  double push_ratio;           /* push a round when its sender arcs * push_ratio <= nnz;
                                  0 = always pull                      */
  int32_t early_exit;          /* coverage-checked pull scans in dense rounds (§3.4)   */
  int32_t arc_mask_permille;   /* filtered pull rounds with >= this many senders per 1000
                                  vertices build the per-arc activity mask first
                                  (0 = always probe per arc)           */
  int32_t prefilter_pct;       /* filtered pull rounds with < this % of vertices sending
                                  probe the in-lists of receivers of in-degree <= 16
                                  lane-parallel first (0 = never)       */
  int32_t compact_rows;        /* 1: 64-word runs keep 128-B compact Message-Lists while
                                  rows are sparse and gather them instead of full rows
                                  (single-rank contexts only)           */
  int32_t unfiltered_pct;      /* pull without the per-arc activity check when >= this %
                                  of vertices are senders (0 = never)   */
  int32_t msg_word_base;       /* message shards: this context's message k
                                  is global message 64*msg_word_base + k; the digest uses
                                  global word indices, so shard digests XOR together     */
  int32_t flat_max_words;      /* rows of at most this many words (<= 32) take the
                                  edge-parallel pull kernel (0 = never)  */
  int64_t summary_min_n;       /* filtered probe rounds of overlays with >= this many
                                  vertices, with at most n/256 senders, probe a summary
                                  level (1 bit per 64 vertices) before the activity
                                  bitmap (0 = never)                    */
  int32_t partition_by_arcs;   /* vertex partitions (gp_set_partition): 0 = slices of equal
                                  vertex count, 1 = slices of equal in-arc count
                                  (set before the partition is made)     */
  int32_t split_deg;           /* degree-split sparse rounds: in a
                                  prefiltered pull without early exit, senders of
                                  in-degree < split_deg push their rows (atomicOr into
                                  the accumulator) and receivers probe only the prefix of
                                  their gather-ordered in-list whose senders have
                                  in-degree >= split_deg (0 = off; single-rank contexts) */
  int32_t split_max_permille;  /* ... only while fewer than this many vertices per 1000
                                  send (default 10: the push half grows with the low-
                                  degree senders; 1000 = whenever prefiltered; ABI 17)   */
} gp_config;

/* what for gp_read */
typedef enum gp_what {
  GP_SEEN = 0,        /* u64 [vend-vbegin][W]  owned rows of the Message-List bitmap */
  GP_FIRST = 1,       /* u8  [vend-vbegin][m]  first-receipt round, 255 = never      */
  GP_DIGEST = 2,      /* u64 [vend-vbegin]                                           */
  GP_COVERAGE = 3,    /* u64 [m]  vertices holding message m (this rank's slice)     */
  GP_FORWARDS = 4,    /* u64 [m]  sends of message m (this rank's senders)           */
  GP_STATE = 5,       /* u8  [n]  bit0 crashed, bit1 removed                         */
  GP_MISS = 6,        /* u8  [n]  heartbeat miss counter                             */
  GP_DEG_LIVE = 7,    /* i32 [n]  neighbours not removed                             */
  GP_ROW_PTR = 8,     /* i64 [n+1] in-CSR offsets (as loaded / built)                */
  GP_COL = 9,         /* i32 [nnz] in-CSR columns                                    */
  GP_FRONTIER = 10,   /* u64 [n][W] current frontier (rows with FPOP==0 read as 0);
                         kept only with track_msg_forwards (else GP_ENOTRACK)      */
  GP_FPOP = 11,       /* u32 [n] |frontier(v)|                                       */
  GP_L2G = 12,        /* i32 [local slots] global id of each local vertex (identity
                         unless partitioned: owned, then ghosts, then origin extras) */
  /* the whole job of a message-shard run, after gp_shard_combine (else GP_ESTATE) */
  GP_JOB_DIGEST = 13,   /* u64 [n]        per-vertex digest of every shard's messages    */
  GP_JOB_COVERAGE = 14, /* u64 [m_total]  vertices holding message k of the job table    */
  GP_JOB_FORWARDS = 15, /* u64 [m_total]  sends of message k (GP_ENOTRACK as GP_FORWARDS) */
  /* per-peer traffic record (gp_track_load below) */
  GP_LOAD_SENT = 16,  /* u64 [n]  gossip lines peer u sent, over all its links       */
  GP_LOAD_RECV = 17,  /* u64 [n]  gossip lines that arrived at peer v, duplicates too */
  GP_SEENPOP = 18,    /* u32 [vend-vbegin]  |Message-List(v)|: the messages v holds
                         (readable without tracking; exact for aliased vertices)   */
  /* per-peer fresh deliveries (gp_track_fresh below) */
  GP_FRESH_SENT = 19, /* u64 [n]  peer u's sends that delivered a first receipt      */
  GP_FRESH_RECV = 20, /* u64 [n]  arrivals at peer v of a message it did not hold    */
  /* per-link fresh deliveries (gp_track_link_fresh below) */
  GP_LINK_FRESH = 21, /* u16 [nnz]  first receipts arc j of the in-CSR delivered     */
  /* per-peer receipt delays (gp_track_delay below) */
  GP_DELAY_SUM = 22,  /* u32 [vend-vbegin]  sum of v's receipt delays, in rounds     */
  GP_DELAY_MAX = 23,  /* u8  [vend-vbegin]  v's largest receipt delay (0: none)      */
  /* delivery multiplicity (gp_track_mult below) */
  GP_SOLE_SENT = 24,  /* u64 [n]  first receipts peer u alone delivered, over its out-arcs */
  GP_SOLE_RECV = 25,  /* u32 [n]  first receipts of peer v that had one deliverer     */
  /* per-peer delay distributions (gp_track_delay_dist below) */
  GP_DELAY_DIST = 26, /* u16 [vend-vbegin][GP_DELAY_DIST_BINS]  v's receipts per delay value */
  /* watched peers (gp_watch below) */
  GP_WATCH_FIRST = 27,   /* u8  [K][m]  first-receipt rows of the watched peers, 255 = never */
  GP_WATCH_ARRIVAL = 28, /* u8  [A][m]  receipt round per watched in-arc and message, 255 = never */
  GP_WATCH_PTR = 29,     /* i64 [K+1]   first watched arc of every slot                      */
  /* delayed links (gp_link_delay below) */
  GP_ARC_DELAY = 30      /* u8  [nnz]   d(u, v) of arc j of the in-CSR, in GP_ROW_PTR / GP_COL order */
} gp_what;

int gp_abi_version(void);
const char* gp_last_error(void);
int gp_device_count(int* n_out);

int gp_create(int device, gp_ctx** out);
void gp_destroy(gp_ctx* ctx);
void gp_default_config(gp_config* cfg);
int gp_configure(gp_ctx* ctx, const gp_config* cfg);

/* Overlay.  In-CSR: row_ptr[v]..row_ptr[v+1] lists u with an arc u->v (the peers
 * whose gossip v receives; Peer.py:402 sends on outgoing links).  out_degree may
 * be NULL for undirected graphs (= in-degree).  For directed graphs the out-CSR
 * (out_row_ptr/out_col, may be NULL when directed == 0) gives the other side of
 * every heartbeat link for liveness reports (Peer.py:369-392 covers outgoing and
 * incoming connections).  A NULL out-CSR of a directed graph is built by
 * transposing the in-CSR; a given one must be its transpose (rows in any
 * order): row_ptr monotone, ids in range and every vertex's out-degree equal
 * to its count in col are checked, GP_EINVAL otherwise. */
int gp_load_graph(gp_ctx* ctx, int64_t n, int64_t nnz, const int64_t* row_ptr,
                  const int32_t* col, int32_t directed, const int64_t* out_row_ptr,
                  const int32_t* out_col);

/* Build an undirected Chung-Lu power-law overlay on the device:
 * ~dbar*n/2 candidate edges, endpoints drawn ∝ (i+1)^(-1/(gamma-1)) with an
 * integer alias table, self-loops dropped, de-duplicated, ids randomly relabelled. */
int gp_build_chung_lu(gp_ctx* ctx, int64_t n, double dbar, double gamma, uint64_t seed);

/* Vertex slice owned by this context (default: all). */
int gp_set_partition(gp_ctx* ctx, int32_t rank, int32_t nranks);
int gp_get_partition(gp_ctx* ctx, int64_t* vbegin, int64_t* vend);

/* RCCL: rank 0 calls gp_comm_unique_id, the host distributes the 128 bytes. */
int gp_comm_unique_id(void* out128);
int gp_comm_init(gp_ctx* ctx, const void* unique_id128, int32_t nranks, int32_t rank);

/* Messages: origin vertex and inject round of each message (Peer.py:397-399:
 * message #n of a peer is its n-th generated gossip). */
int gp_set_messages(gp_ctx* ctx, int32_t m, const int32_t* origin, const int32_t* inject_round);

/* Spread keys of candidate origins, for ordering a message table before
 * gp_set_messages (DESIGN.md §3.4 "message order"; no reference counterpart:
 * the reference's Message-List is an unordered set of strings, Peer.py:175-216,
 * so the bit position of a message is the engine's choice).  keys_out[k] is the
 * number of arc endpoints within `hops` (1..3) of origin[k]: hops 1 = degree,
 * 2 = the sum of its neighbours' degrees, 3 = the sum over its neighbours of
 * their hops-2 key.  Messages whose keys are close spread at similar speed, so
 * placing them in adjacent bits lets the late early-exit rounds skip whole
 * 128-B lines of Message-List rows.  Needs the global overlay (before
 * gp_set_partition with nranks > 1). */
int gp_spread_keys(gp_ctx* ctx, int32_t hops, int32_t m, const int32_t* origin, uint64_t* keys_out);

/* Explicit crash injection (the reference's silent mode, Peer.py:437-439),
 * applied at the start of the next round in addition to random churn. */
int gp_crash(gp_ctx* ctx, int32_t nverts, const int32_t* verts);

int gp_reset(gp_ctx* ctx);                       /* new run: clear all per-run state */
int gp_round(gp_ctx* ctx, gp_round_stats* out);  /* liveness + injection + expansion */
int gp_run(gp_ctx* ctx, int32_t max_rounds, gp_round_stats* per_round, int32_t* rounds_out);
/* Single-process multi-context round: ctxs[k] owns partition k of nctx (same or
 * different devices, no RCCL); the exchange is device-to-device copies and the
 * counters are summed into *out.  Used for partition-invariance checks on one GPU. */
int gp_round_group(gp_ctx** ctxs, int32_t nctx, gp_round_stats* out);
/* Per-message coverage / forwards of the run so far.  Without liveness and
 * track_msg_forwards the forwards come from the Message-Lists (every holder sent
 * once to each link); in a run that stopped before quiescence -- the round
 * limit, or a caller that stops -- the last round's receivers have not sent
 * yet: their frontier rows come off again where the context keeps them, and
 * where it keeps none GP_FORWARDS / GP_JOB_FORWARDS answer GP_ENOTRACK. */
int gp_finalize_messages(gp_ctx* ctx);
int gp_read(gp_ctx* ctx, int32_t what, void* host, int64_t bytes);
int gp_reports(gp_ctx* ctx, gp_report* buf, int64_t cap, int64_t* n_out);
int gp_synchronize(gp_ctx* ctx);
int gp_info(gp_ctx* ctx, int64_t* n, int64_t* nnz, int32_t* m, int32_t* words);
/* Local shape of a (partitioned) context: owned vertices, ghosts, origin
 * extras, arcs of the local CSR, boundary entries it sends to (all peers). */
int gp_local_info(gp_ctx* ctx, int64_t* nloc, int64_t* nghost, int64_t* nextra, int64_t* nnz_local,
                  int64_t* n_boundary);

/* Message-shard jobs.  Messages never interact, so an N-GPU
 * job runs one context per GPU on the whole overlay, rank p holding the
 * word-aligned block of the message table that starts at global word
 * gp_config.msg_word_base.  The reference keeps each peer's whole receive
 * record (Peer.py:175-216); gp_shard_combine makes the job's record out of the
 * ranks' after gp_run: the per-vertex digests XOR-reduced (reduce-scatter by
 * ncclSend/ncclRecv of 1/N vertex slices + an XOR kernel, then ncclAllGather),
 * the per-message coverage / forwards all-gathered into the job's message
 * order, and the per-round counters: additive ones summed, `receivers` and
 * `active` as the popcount of the OR of the ranks' per-round vertex bitmaps
 * (reduce-scattered like the digests: a vertex receiving in two shards counts
 * once), liveness counters checked equal across ranks.  Every rank gets the
 * same job record.
 *
 * The transport is a communicator of the shard ranks (gp_shard_comm_init: one
 * GPU per rank), or the host's own all-gather (gp_shard_host_init: ranks
 * sharing a GPU, which RCCL refuses -- the rehearsal of a one-GPU box; the
 * reductions still run on the device).  Rounds of a shard job take no
 * collective: each rank decides its own direction / scan modes.  A shard job
 * records two n-bit bitmaps per round (exchange_ms of gp_round_stats). */
typedef int (*gp_allgather_fn)(void* user, const void* send, int64_t bytes, void* recv);   /* recv: [nranks][bytes] */
int gp_shard_comm_init(gp_ctx* ctx, const void* unique_id128, int32_t nranks, int32_t rank);
int gp_shard_host_init(gp_ctx* ctx, gp_allgather_fn fn, void* user, int32_t nranks, int32_t rank);
/* the communicator's own count and rank (ncclCommCount / ncclCommUserRank), or
 * those given to gp_shard_host_init; transport_out: 1 = RCCL, 2 = host */
int gp_shard_info(gp_ctx* ctx, int32_t* nranks_out, int32_t* rank_out, int32_t* transport_out);
/* after gp_run (uninterrupted since gp_reset) on every rank; finalizes first if
 * needed.  job[0..*rounds_out) = the job's per-round counters (cap >= rounds);
 * *ms_out (may be NULL) = device time of the combine on the engine stream. */
int gp_shard_combine(gp_ctx* ctx, gp_round_stats* job, int32_t cap, int32_t* rounds_out, double* ms_out);

/* Spread curves: curve[r][k] = the vertices whose first receipt of message k
 * has receipt round r -- column by column the histogram of the first-receipt
 * matrix (GP_FIRST), kept at sizes where that matrix cannot be (DESIGN.md
 * §3.7).  It is the aggregate of what each reference peer logs per arrival
 * (Peer.py:175-216: every received gossip with its time).  An origin's own
 * receipt at its inject round counts; a lost message counts nowhere; a vertex-
 * partitioned context counts its owned vertices, as GP_COVERAGE does.
 *
 * gp_track_curve(on) takes effect at the next gp_reset, which makes the
 * allocations: the exact frontier rows (2 x n x 8W bytes, as with
 * track_msg_forwards) and a [255][64W] u64 count buffer.  Tracking adds a
 * counting pass after each round's expansion (round_ms carries it; expand_ms
 * and kernel_ms keep their meaning); it changes no other output and makes
 * neither GP_FRONTIER nor GP_FORWARDS readable where they were not.
 *
 * gp_read_curve writes u64 [rows][m] (the m real columns) and *rows_out = rows.
 * job = 0: this context's curve, rows = rounds run since gp_reset + 1; row R
 * holds the receipts round R-1's expansion produced (round R's injections are
 * not made yet).  GP_ENOTRACK before tracking took effect; GP_ESTATE for a run
 * restored from a checkpoint past round 0 (the blob does not hold the curve),
 * until the next gp_reset.  job = 1: the whole shard job's curve after
 * gp_shard_combine (else GP_ESTATE), the ranks' curves at their blocks of the
 * job's message order, rows = the job's rounds + 1; GP_ENOTRACK unless every
 * rank tracked a valid curve.  GP_EINVAL if cap_rows < rows: nothing is written. */
int gp_track_curve(gp_ctx* ctx, int32_t on);
int gp_read_curve(gp_ctx* ctx, int32_t job, uint64_t* host, int32_t cap_rows, int32_t* rows_out);

/* Per-peer traffic record: the totals of what every
 * reference peer logs line by line -- Peer.py:206 and Peer.py:286 log each
 * arriving message with the peer it came from, duplicate or not, and
 * Peer.py:402-404 send on every outgoing link.  Over the rounds run since
 * gp_reset, with frontier_r(u) u's frontier after the liveness and injection
 * phases of round r (empty for a vertex that is down):
 *   GP_LOAD_SENT  sent[u] = sum_r max(deg_live_r(u), 0) * |frontier_r(u)|, the
 *                 sends gp_round_stats.sends counts, per sender: the array sums
 *                 to the sum of the rounds' sends exactly;
 *   GP_LOAD_RECV  recv[v] = sum_r [v up in round r] * sum_{u in In(v)}
 *                 |frontier_r(u)|.  A send to a crashed, not yet removed peer is
 *                 attempted: it counts in sent and is received by nobody; a
 *                 link to a removed peer carries nothing.  So sum recv <= sum
 *                 sent, with equality when no vertex is ever down.
 * recv[v] - (GP_SEENPOP[v] - messages injected at v) are v's duplicate arrivals.
 * Both are readable between rounds.  A context that runs a block of a message
 * table (msg_word_base) holds the totals of its own messages: the arrays of a
 * job's shards add up to the whole run's (the host adds them; gp_shard_combine
 * does not).
 *
 * gp_track_load(on) takes effect at the next gp_reset, which allocates (and
 * clears) two u64[n] and one u32[n]; off, nothing is allocated or launched.
 * While no vertex has ever been down the rounds launch nothing either: a read
 * computes the totals from the run's state (every message a vertex holds was in
 * its frontier exactly once), one pass over the in-CSR.  With churn, or from
 * the first gp_crash on (which books the rounds so far before it is applied),
 * every round adds its own pass before the expansion (round_ms carries it;
 * expand_ms and kernel_ms keep their meaning).  GP_LOAD_EAGER=1 in the
 * environment at gp_create counts per round from round 0 (a test lever).
 * Tracking changes no other output.
 *
 * Reads: GP_ENOTRACK before tracking took effect, and on a vertex-partitioned
 * context (nranks > 1: ghosts keep no frontier counts -- not supported);
 * GP_ESTATE for a run that counts per round and was restored from a checkpoint
 * past round 0 (the blob does not hold the totals), until the next gp_reset.  A
 * restored run that never had a vertex down reads correctly: its totals are a
 * function of the restored state. */
int gp_track_load(gp_ctx* ctx, int32_t on);

/* Per-peer fresh deliveries: of the lines the traffic
 * record counts, the ones that told the receiver something it did not hold --
 * what one reads a gossip log (Peer.py:206, Peer.py:286: every arrival with
 * the peer it came from) for.  With frontier_r(u) as above and new_r(v) the
 * messages v first receives in the expansion of round r (receipt round r + 1),
 * over the rounds run since gp_reset:
 *   GP_FRESH_SENT  fresh_sent[u] = sum_r sum_{v in Out(u)} |frontier_r(u) & new_r(v)|,
 *                  u's sends that delivered a first receipt;
 *   GP_FRESH_RECV  fresh_recv[v] = sum_r sum_{u in In(v)}  |frontier_r(u) & new_r(v)|,
 *                  the arrivals at v of a message v did not hold at the start
 *                  of the round.
 * Several in-neighbours delivering one message in the same round all count:
 * none was a duplicate when it was sent.  A down receiver has no new_r, a
 * crashed sender's frontier is dropped, a removed peer is down.  So
 *   sum fresh_sent = sum fresh_recv exactly;
 *   fresh_sent[u] <= GP_LOAD_SENT[u] and fresh_recv[v] <= GP_LOAD_RECV[v]
 *   (sent - fresh_sent: u's wasted sends; recv - fresh_recv: v's stale arrivals);
 *   fresh_recv[v] >= GP_SEENPOP[v] - messages injected at v, with equality iff
 *   every message reached v from one neighbour only;
 *   per round, sum fresh_recv grows by at least gp_round_stats.new_bits.
 * Both are pure functions of the first-receipt matrix: arc u -> v contributes
 * the messages m with first[v][m] = first[u][m] + 1 and u up in round
 * first[u][m].  Readable between rounds.  A context that runs a block of a
 * message table (msg_word_base) holds the totals of its own messages: the
 * arrays of a job's shards add up to the whole run's (the host adds them;
 * gp_shard_combine does not).
 *
 * gp_track_fresh(on) takes effect at the next gp_reset, which makes the exact
 * frontier rows exist (the buffers track_msg_forwards and gp_track_curve keep,
 * shared when several are on) and allocates (and clears) two u64[n]; off,
 * nothing is allocated or launched.  Every round then adds one pass after the
 * expansion (round_ms carries it; expand_ms and kernel_ms keep their meaning).
 * Tracking changes no other output and no counter; it does not make
 * GP_FRONTIER or GP_FORWARDS readable and does not turn on the per-round
 * forwards pass.  GP_FRESH_GATHER=1 in the environment at gp_create runs
 * undirected overlays through the pass's other form, one gather per role and
 * no per-arc atomics (a measurement lever; the totals are the same).
 *
 * Reads: GP_ENOTRACK before tracking took effect, and on a vertex-partitioned
 * context (nranks > 1: not supported); GP_ESTATE for a run restored from a
 * checkpoint past round 0 (the blob does not hold the totals, and they are no
 * function of the restored state), until the next gp_reset. */
int gp_track_fresh(gp_ctx* ctx, int32_t on);

/* Fresh-delivery curves: the fresh deliveries split by
 * message and round instead of by peer -- for message k in round r, how many
 * of the sends that carried it delivered a first receipt.  With frontier_r(u)
 * and new_r(v) as above,
 *   fresh_curve[r + 1][k] = #{ arcs u -> v, u in In(v) : k in frontier_r(u) & new_r(v) }
 *   fresh_curve[0][k]     = 0
 * rows indexed by receipt round, so that they line up with the spread curve's:
 * fresh_curve[R][k] / curve[R][k] is the deliverers per first receipt of
 * message k at receipt round R.  Several in-neighbours delivering k to v in one
 * round all count, with no tie-break; an injection has no deliverer; a down
 * receiver has no new_r, a crashed sender's frontier is dropped, a removed peer
 * is down.  So
 *   the sum of row r + 1 is what sum GP_FRESH_RECV grows by in round r, exactly;
 *   the column sums are the run's news deliveries of each message, and the
 *   whole array sums to sum GP_FRESH_RECV = sum GP_FRESH_SENT;
 *   fresh_curve[R][k] >= curve[R][k] - (injections of k at round R at an up
 *   origin) for R >= 1: every expansion receipt has at least one deliverer;
 *   fresh_curve[R][k] <= the sends of message k in round R - 1.
 * It is a pure function of the first-receipt matrix: arc u -> v counts for
 * column k at row first[u][k] + 1 iff first[u][k] != 255, first[v][k] =
 * first[u][k] + 1 and u is up in round first[u][k].  A context that runs a
 * block of a message table (msg_word_base) holds the columns of its own
 * messages: the shards' arrays concatenate to the whole run's (the host does
 * it; gp_shard_combine does not).
 *
 * gp_track_fresh_curve(on) takes effect at the next gp_reset, which makes the
 * exact frontier rows exist (shared with track_msg_forwards, gp_track_curve and
 * gp_track_fresh when several are on) and allocates (and clears) a [255][64W]
 * u64 buffer; off, nothing is allocated or launched.  Every round then adds
 * one pass after the expansion (round_ms carries it; expand_ms and kernel_ms
 * keep their meaning); a round whose receipt round would be 255 or more is
 * refused, as with gp_track_curve.  Tracking changes no other output and no
 * counter, and makes neither GP_FRONTIER nor GP_FORWARDS readable.  An overlay
 * of 2^32 arcs or more is refused at that gp_reset (GP_EINVAL).
 * GP_FRESH_CURVE_GRID=blocks in the environment at gp_create caps the pass's
 * grid (a test lever; the array is the same).
 *
 * gp_read_fresh_curve writes u64 [rows][m] (the m real columns) and *rows_out =
 * rows = rounds run since gp_reset + 1.  Readable between rounds; a read
 * changes nothing.  GP_EINVAL for a null argument or cap_rows < rows: nothing
 * is written.  GP_ENOTRACK before tracking took effect, and on a vertex-
 * partitioned context (nranks > 1: not supported); GP_ESTATE for a run restored
 * from a checkpoint past round 0 (the blob does not hold the record), until the
 * next gp_reset. */
int gp_track_fresh_curve(gp_ctx* ctx, int32_t on);
int gp_read_fresh_curve(gp_ctx* ctx, uint64_t* host, int32_t cap_rows, int32_t* rows_out);

/* Per-link fresh deliveries: the fresh deliveries per
 * overlay link -- the arrival lines of a gossip log (Peer.py:206, Peer.py:286)
 * that were news, grouped by the connection they came over.  For arc j of the
 * in-CSR as loaded or built (GP_ROW_PTR / GP_COL), row_ptr[v] <= j <
 * row_ptr[v + 1] and u = col[j], so sender u and receiver v, over the rounds
 * run since gp_reset:
 *   GP_LINK_FRESH  link_fresh[j] = sum_r |frontier_r(u) & new_r(v)|
 * Several in-neighbours delivering one message in the same round all count,
 * with no tie-break; an injection has no deliverer; a down receiver has no
 * new_r, a crashed sender's frontier is dropped, a removed peer is down.  It is
 * a pure function of the first-receipt matrix: arc u -> v counts message m iff
 * first[u][m] != 255, first[v][m] = first[u][m] + 1 and u is up in round
 * first[u][m].  So, all exactly,
 *   the sum over the arcs of row v is GP_FRESH_RECV[v];
 *   the sum over the arcs with col[j] = u is GP_FRESH_SENT[u];
 *   the whole array sums to sum GP_FRESH_RECV = the sum of the fresh-delivery curve.
 * link_fresh[j] <= m <= 4096, because v first receives each message once: the
 * record is u16 per arc.  The bound is attained (a path with every message
 * injected at one end: 4096 on the arcs pointing away from it, 0 on the arcs
 * pointing back).  An undirected link is two arcs, u -> v and v -> u, counted
 * separately (links.undirected of the Python package folds them).  Readable
 * between rounds.  A context that runs a block of a message table
 * (msg_word_base) holds the counts of its own messages: the shards' arrays add
 * up element by element to the whole run's (the host adds them;
 * gp_shard_combine does not).
 *
 * gp_read_link_hist computes, on the device and from the current record,
 * link_hist[c] = the number of arcs with link_fresh = c for c = 0 .. 4096:
 * link_hist[0] is the idle arcs, and the fewest arcs that carry a given share
 * of the news follow from the histogram alone, without reading the array.
 * `bins` must be 4097 (else GP_EINVAL, nothing written).  The histograms of a
 * job's shards do not add up to the whole run's.
 *
 * gp_track_link_fresh(on) takes effect at the next gp_reset, which makes the
 * exact frontier rows exist (shared with track_msg_forwards and the other
 * records when several are on) and allocates (and clears) the u16[nnz]; off,
 * nothing is allocated or launched, and turning it off frees the array at the
 * next gp_reset.  Loading another overlay re-sizes it.  Every round then adds
 * one pass after the expansion (round_ms carries it; expand_ms and kernel_ms
 * keep their meaning).  Tracking changes no other output and no counter, the
 * work counters included, and makes neither GP_FRONTIER nor GP_FORWARDS
 * readable.
 *
 * Reads (gp_read GP_LINK_FRESH and gp_read_link_hist): GP_ENOTRACK before
 * tracking took effect, and on a vertex-partitioned context (nranks > 1: not
 * supported); GP_ESTATE for a run restored from a checkpoint past round 0 (the
 * blob does not hold the record), until the next gp_reset; GP_EINVAL on a
 * byte-count mismatch (expected 2 * nnz). */
int gp_track_link_fresh(gp_ctx* ctx, int32_t on);
int gp_read_link_hist(gp_ctx* ctx, uint64_t* hist, int32_t bins);

/* Per-peer receipt delays: how late every peer hears
 * the news -- the arrival lines of a gossip log carry their time (Peer.py:206,
 * Peer.py:286); grouped by the receiving peer they say how long after a
 * message was generated that peer heard it.  For an owned vertex v, over the
 * messages k of the context's table:
 *   GP_DELAY_SUM  delay_sum[v] = sum_{k : first[v][k] != 255} (first[v][k] - inject_round[k])
 *   GP_DELAY_MAX  delay_max[v] = max_{k : first[v][k] != 255} (first[v][k] - inject_round[k]),
 *                 0 if v holds nothing
 * GP_SEENPOP[v] is the number of terms: the mean delay is delay_sum / seenpop,
 * and a peer with seenpop = 0 was never reached (delay_max = 0 alone does not
 * say so: an origin that only holds its own messages has it too).  An injection
 * at an up origin is a receipt with delay 0.  A receipt of round r's expansion
 * has receipt round r + 1 and delay r + 1 - inject_round[k] >= 1; it counts when
 * it happens, so a receiver that crashes in round r + 1 still received.  In the
 * round-synchronous model a delay is the receiver's hop distance from the
 * origin on the live overlay: the mean is a sampled closeness, the maximum a
 * sampled eccentricity.  Both arrays are pure functions of the first-receipt
 * matrix and the message table.  delay_max <= 254 (inject_round <= 253, rounds
 * stop at 253) and delay_sum <= 4096 * 254 < 2^21.  Over a single-rank run,
 *   sum_v delay_sum[v] = sum_R sum_k (R - inject_round[k]) * curve[R][k], exactly.
 * The arrays hold totals since gp_reset and are readable between rounds: after
 * R rounds, the receipts with first <= R.  A context that runs a block of a
 * message table (msg_word_base) holds its own messages' terms: the shards'
 * delay_sum arrays add up and delay_max is their element-wise maximum (the
 * host combines them; gp_shard_combine does not).  A vertex-partitioned
 * context keeps the record for its owned vertices, read as [vend - vbegin]
 * like GP_SEENPOP.
 *
 * gp_read_delay_bins computes, on the device and from the current record, the
 * delays by degree: a u64 [GP_DELAY_BINS][GP_DELAY_COLS] table whose row b
 * holds the owned vertices with bin(deg) = b, where deg is the vertex's
 * in-list length in the context's CSR and bin(deg) = 0 for deg <= 1, else
 * floor(log2(deg)).  Columns: peers; peers reached (seenpop > 0); receipts
 * (sum seenpop); sum delay_sum; max delay_max.  Over shards or partition
 * ranks, columns 0-3 add where the vertex sets are disjoint (over shards of one
 * vertex set columns 2-3 add), and column 4 takes the maximum.  `bins` must be
 * GP_DELAY_BINS (else GP_EINVAL, nothing written).
 *
 * gp_track_delay(on) takes effect at the next gp_reset, which allocates (and
 * clears) 5 bytes per owned vertex; off, nothing is allocated or launched, and
 * turning it off frees the arrays at the next gp_reset.  Every round then adds
 * one pass after the expansion (round_ms carries it; expand_ms and kernel_ms
 * keep their meaning): over the receivers' own new rows -- the exact frontier
 * rows, which the reset makes exist -- or, when every message of the table has
 * the same inject round, over the per-vertex counts alone: such a table keeps
 * no frontier rows for this record (GP_DELAY_ROWS=1 in the environment at
 * gp_create takes the row pass, and keeps the rows, for such a table too: a
 * test and measurement lever, same arrays).  Tracking changes no other output and no
 * counter, and makes neither GP_FRONTIER nor GP_FORWARDS readable.
 *
 * Reads (gp_read GP_DELAY_SUM / GP_DELAY_MAX and gp_read_delay_bins):
 * GP_ENOTRACK before tracking took effect; GP_ESTATE for a run restored from a
 * checkpoint past round 0 (the blob does not hold the record), until the next
 * gp_reset; GP_EINVAL on a byte-count mismatch (expected 4 or 1 per owned
 * vertex), a bin-count mismatch or a null argument. */
#define GP_DELAY_BINS 32
#define GP_DELAY_COLS 5
int gp_track_delay(gp_ctx* ctx, int32_t on);
int gp_read_delay_bins(gp_ctx* ctx, uint64_t* out, int32_t bins);

/* Per-peer delay distributions: the same receipts per
 * delay value, so that a peer's median and tail can be read, not its mean and
 * maximum alone.  For an owned vertex v, over the messages k of the context's
 * table, with D = GP_DELAY_DIST_BINS:
 *   GP_DELAY_DIST  delay_dist[v][d] = #{ k : first[v][k] != 255,
 *                  min(first[v][k] - inject_round[k], D - 1) = d }     u16 [vend - vbegin][D]
 * Columns 1 .. D - 2 are exact, column D - 1 is "D - 1 rounds or later", column 0
 * holds the receipts with delay 0: the injections at v at an up origin.  Every
 * cell is <= m <= 4096.  sum_d delay_dist[v][d] = GP_SEENPOP[v] at every read
 * between rounds: column 0 is computed by the reads, on the device, as seenpop
 * minus the other columns.  With gp_track_delay also on, a peer with an empty
 * last column has sum_d d * delay_dist[v][d] = delay_sum[v] and its largest
 * occupied column is delay_max[v]; otherwise the weighted sum (the last column
 * at D - 1) is <= delay_sum[v] and delay_max[v] >= D - 1.  Over a single-rank
 * run with gp_track_curve the column sums are the run's receipts per delay.
 * Expansion receipts count when they happen (a receiver that crashes in the
 * next round still received).  Scope as the receipt delays': totals since
 * gp_reset, readable between rounds; a context that runs a block of a message
 * table holds its own messages' receipts and the shards' arrays add element by
 * element (the host adds them, in a wider type); a vertex-partitioned context
 * keeps the record for its owned vertices.
 *
 * gp_read_delay_dist_bins computes, on the device and from the current record,
 * a u64 [GP_DELAY_BINS][GP_DELAY_DIST_BINS] table: row b sums the rows of the
 * owned vertices with bin(in-list length) = b (gp_read_delay_bins' bins),
 * column 0 included; sum_d table[b][d] is gp_read_delay_bins' receipts column.
 * `bins` must be GP_DELAY_BINS (else GP_EINVAL, nothing written).
 *
 * gp_track_delay_dist(on) takes effect at the next gp_reset, which allocates
 * (and clears) 32 bytes per owned vertex; off, nothing is allocated or
 * launched, and turning it off frees the array at the next gp_reset.  It is
 * independent of gp_track_delay: either, both or neither.  Every round then
 * adds one pass after the expansion, over the receivers' own new rows or, when
 * every message of the table has the same inject round, over the per-vertex
 * counts alone: such a table keeps no frontier rows for this record
 * (GP_DELAY_ROWS=1 takes the row pass here too).
 *
 * Reads: GP_ENOTRACK before tracking took effect; GP_ESTATE for a run restored
 * from a checkpoint past round 0, until the next gp_reset; GP_EINVAL on a
 * byte-count mismatch (expected 2 * GP_DELAY_DIST_BINS per owned vertex), a
 * bin-count mismatch or a null argument. */
#define GP_DELAY_DIST_BINS 16
int gp_track_delay_dist(gp_ctx* ctx, int32_t on);
int gp_read_delay_dist_bins(gp_ctx* ctx, uint64_t* out, int32_t bins);

/* Delivery multiplicity: how fragile the flood was.
 * The fresh-delivery records are sums over deliverers; this one keeps the
 * number of deliverers behind each first receipt -- the arrival lines of one
 * message at one peer in the round it was news (Peer.py:206, Peer.py:286).  A
 * receipt with ten deliverers survives nine crashed neighbours; a receipt with
 * one hangs on a single link and a single peer.  With frontier_r(u) and
 * new_r(v) as for the fresh deliveries, for k in new_r(v)
 *   mult_r(v, k) = #{ arcs j of row v of the in-CSR : k in frontier_r(col[j]) }  >= 1
 * (parallel arcs count separately; no tie-break is involved; an injection at an
 * up origin is a receipt with no deliverer).  Over the rounds since gp_reset:
 *   gp_read_mult_hist  u64 [GP_MULT_BINS]: hist[c], c = 1 .. 15, the first
 *                 receipts with exactly c deliverers; hist[16] those with 16 or
 *                 more; hist[0] the injections at up origins (taken from the
 *                 rounds' `injected` counters)
 *   GP_SOLE_RECV  sole_recv[v]: v's receipts with mult = 1 (<= m <= 4096)
 *   GP_SOLE_SENT  sole_sent[u]: the receipts, over all of u's out-arcs, for
 *                 which u was the only deliverer -- the news that would have
 *                 arrived later or never without u
 *   gp_read_sole_bins  u64 [GP_SOLE_BINS][GP_SOLE_COLS], computed on the device
 *                 from the current record: row b holds the vertices with
 *                 bin(in-list length) = b (gp_read_delay_bins' bins); columns:
 *                 peers; receipts (sum GP_SEENPOP); sum sole_recv; sum sole_sent
 * From the first-receipt matrix: for first[v][k] != 255 the deliverers are the
 * arcs u -> v with first[u][k] != 255, first[v][k] = first[u][k] + 1 and u up
 * in round first[u][k]; c is their number, and c = 0 iff the receipt is the
 * injection.  Exactly:
 *   sum_c hist[c] = sum_k coverage[k] (single rank, after gp_finalize),
 *   sum_{c >= 1} hist[c] = sum_r stats[r].new_bits,
 *   hist[1] = sum sole_recv = sum sole_sent,
 *   sole_recv[v] <= GP_SEENPOP[v] - (messages injected at v),
 * and with gp_track_fresh as well sole_recv <= fresh_recv, sole_sent <=
 * fresh_sent element by element and sum_{c <= 15} c * hist[c] + 16 * hist[16]
 * <= sum fresh_recv.  The arrays hold totals since gp_reset and are readable
 * between rounds: after R rounds, the receipts with first <= R.  A context
 * that runs a block of a message table (msg_word_base) holds its own messages'
 * receipts: the shards' three arrays, the histogram included, add up element
 * by element (the host adds them; gp_shard_combine does not).
 *
 * gp_track_mult(on) takes effect at the next gp_reset, which makes the exact
 * frontier rows exist and allocates (and clears) 12 bytes per vertex plus the
 * hubs' scratch (5 rows per hub item and one per hub, 8 * W bytes each); off,
 * nothing is allocated or launched, and turning it off frees everything at the
 * next gp_reset.  Every round then adds one pass after the expansion (round_ms
 * carries it; expand_ms and kernel_ms keep their meaning).  Tracking changes
 * no other output and no counter, and makes neither GP_FRONTIER nor
 * GP_FORWARDS readable.
 *
 * Reads (gp_read GP_SOLE_SENT / GP_SOLE_RECV, gp_read_mult_hist,
 * gp_read_sole_bins): GP_ENOTRACK before tracking took effect, and on a
 * vertex-partitioned context (not supported); GP_ESTATE for a run restored
 * from a checkpoint past round 0 (the blob does not hold the record), until
 * the next gp_reset; GP_EINVAL on a byte-count mismatch (expected 8 or 4 per
 * vertex), a bin-count mismatch or a null argument, with nothing written. */
#define GP_MULT_BINS 17
#define GP_SOLE_BINS 32
#define GP_SOLE_COLS 4
int gp_track_mult(gp_ctx* ctx, int32_t on);
int gp_read_mult_hist(gp_ctx* ctx, uint64_t* hist, int32_t bins);
int gp_read_sole_bins(gp_ctx* ctx, uint64_t* out, int32_t bins);

/* Watched peers: the arrival log of a caller-chosen
 * list of peers, link by link.  The reference's user-facing output is a log per
 * peer: every gossip line that arrives is written down with the peer it came
 * from and the time (Peer.py:206, Peer.py:286, through Peer.log, Peer.py:40-47).
 * Forward-once means a sender puts each message on a link exactly once, so the
 * whole arrival log of peer v is a [deg_in(v)][m] byte matrix: the round in which
 * that link delivered that message, or never.
 *
 * The watch list is v_0 .. v_{K-1}: distinct global vertex ids in the caller's
 * order; s is a peer's slot, A = sum_s deg_in(v_s), and watched arc
 * a = watch_ptr[s] + i is the i-th arc of row v_s of the in-CSR as loaded or
 * built (GP_ROW_PTR / GP_COL, GP_LINK_FRESH's indexing), with sender
 * u = col[row_ptr[v_s] + i]:
 *   GP_WATCH_FIRST    watch_first[s][k]   = first[v_s][k]                   u8 [K][m]
 *   GP_WATCH_ARRIVAL  watch_arrival[a][k] = r + 1  if k in frontier_r(u)
 *                                                  and v_s is up in E_r     u8 [A][m]
 *   GP_WATCH_PTR      watch_ptr[s]                                          i64 [K + 1]
 * 255 = never; a cell is the receipt round (<= 254), as in GP_FIRST, and is
 * unique: u's frontier holds k in at most one round.  A line is fresh iff
 * watch_arrival[a][k] == watch_first[s][k]; otherwise it is a duplicate and
 * arrived later.  From the first-receipt matrix: watch_arrival[a][k] =
 * first[u][k] + 1 iff first[u][k] != 255 and both u and v_s are up in round
 * first[u][k]; a crashed sender's frontier is dropped, a send to a crashed
 * watched peer arrives nowhere.  On a raw CSR parallel arcs are separate rows
 * with equal contents and a self-loop is a row of duplicates.  Per watched
 * peer, exactly: the cells != 255 count GP_LOAD_RECV[v_s], the fresh ones
 * GP_FRESH_RECV[v_s] and per arc GP_LINK_FRESH[j], the messages with exactly
 * one fresh arc GP_SOLE_RECV[v_s], and watch_first[s] is GP_FIRST's row.
 *
 * Scope: totals since gp_reset, readable between rounds (after R rounds the
 * cells with value <= R; an injection of round R is not in it yet).  A context
 * that runs a block of a message table (msg_word_base) holds its own messages'
 * columns: the shards' arrays concatenate along k.  A vertex-partitioned
 * context does not keep the record.  It is not in the checkpoint blob.
 * Watching changes no other output; it makes the context keep the exact
 * frontier rows, as gp_track_fresh does.
 *
 * gp_watch sets the list for the next gp_reset (count = 0: none; the record is
 * then freed at that reset).  max_bytes bounds the two byte arrays, 0 meaning
 * 1 GiB.  Checked at the call against the overlay then loaded: GP_ESTATE without
 * one; GP_EINVAL for an id outside [0, n), a repeated id or count >
 * GP_WATCH_MAX_PEERS; GP_ENOMEM when (A + K) * 64 W bytes, at the row width W
 * the message table then has, exceed max_bytes -- gp_last_error names the size
 * (gp_reset checks again if the table changed since).  A refused call leaves
 * the previous list in force.  Loading another overlay drops the list.
 * gp_watch_info reports the list in force for the current run (peers, arcs,
 * bytes of the two arrays; 0s when none is); any pointer may be null.
 *
 * Reads: gp_read with the three kinds above (columns are the m real messages),
 * and gp_read_watch_peer for one slot's [m] and [deg][m] (arrival_bytes must
 * be deg * m), so that one hub's log does not cost a download of the whole
 * record.  GP_ENOTRACK before the list has taken effect, and on a vertex-
 * partitioned context; GP_ESTATE for a run restored from a checkpoint past
 * round 0, until the next gp_reset; GP_EINVAL on a byte-count mismatch, a slot
 * outside [0, K) or a null argument. */
#define GP_WATCH_MAX_PEERS 65536
int gp_watch(gp_ctx* ctx, int32_t count, const int32_t* verts, int64_t max_bytes);
int gp_watch_info(gp_ctx* ctx, int32_t* count, int64_t* arcs, int64_t* bytes);
int gp_read_watch_peer(gp_ctx* ctx, int32_t slot, void* first_row, void* arrival, int64_t arrival_bytes);

/* Lossy links (csrc/lossy.hip, csrc/link_loss.h).
 * The flood of §2.2 delivers every line put on an arc.  With loss on, the line
 * u puts on arc u -> v in round r arrives iff
 *
 *   draw(stream_key(seed, 0x200 + r), ((uint64_t)u << 32) | v) >= thresh
 *
 * with thresh = (uint64_t)ldexp(p, 64) for 0 < p < 1; p = 0 leaves every arc
 * open, p = 1 closes every arc.  u and v are global vertex ids.  The draw
 * belongs to the ordered pair and the round: it is the same for every message
 * and every row width, independent for u -> v and v -> u, and parallel arcs of
 * a raw CSR share it.  A vertex still sends a message only in the one round
 * after its first receipt, so a line on a closed arc is lost for good: there
 * is no retransmission.  `sends` and GP_FORWARDS stay the *attempted* sends;
 * termination, injection, liveness and the digest (a function of the
 * first-receipt matrix) are unchanged, and heartbeats are never dropped.  A
 * message table run in blocks (msg_word_base) gives exactly the columns of
 * the whole run, and no gp_config tuning field changes an output.  Coverage
 * is NOT monotone in p for a fixed seed: receiving earlier moves a peer's one
 * forwarding round onto another set of open arcs.
 *
 * gp_link_loss sets the request for the next gp_reset (on = 0: off; p and
 * seed are then ignored beyond the range check).  GP_EINVAL for p < 0, p > 1
 * or NaN: the previous request stays.  gp_link_loss_info reports the setting
 * in force for the current run (any pointer may be null).
 *
 * gp_reset fails with GP_EINVAL, and changes nothing, when loss is requested
 * together with a record that walks arcs -- gp_track_load, gp_track_fresh,
 * gp_track_fresh_curve, gp_track_link_fresh, gp_track_mult, gp_watch (they
 * would count closed arcs as deliveries; gp_last_error names the record) -- or
 * in a vertex-partitioned context.  The records that read only the receivers'
 * new rows stay exact: gp_track_curve, gp_track_delay, gp_track_delay_dist,
 * track_first, track_digest, track_msg_forwards, coverage and forwards.
 *
 * Loss makes the context keep the exact frontier rows (as gp_track_fresh
 * does): the lossy expansion reads them, not whole Message-Lists.  Its rounds
 * report gp_round_stats.mode = 2 and scan = 0.
 *
 * Checkpoints: the blob does not record the loss setting.  The draw depends on
 * the round number alone, so a blob loaded into a context with the same
 * gp_link_loss setting (made before that context's gp_reset) continues
 * bit-exactly; repeating the setting is the caller's job. */
int gp_link_loss(gp_ctx* ctx, int32_t on, double p, uint64_t seed);
int gp_link_loss_info(gp_ctx* ctx, int32_t* on, double* p, uint64_t* seed);

/* Delayed links (csrc/delayed.hip, csrc/link_delay.h; DESIGN.md §2.2, §2.6,
 * §3.19).  The flood of §2.2 crosses every link in one round.  With delay on,
 * the link between u and v takes
 *
 *   d(u, v) = 1 + below(draw(stream_key(seed, 0x300),
 *                            ((uint64_t)min(u, v) << 32) | max(u, v)), dmax)
 *
 * rounds, dmax in [1, 8], u and v global vertex ids: the line u sends in round
 * s (it still sends a message only in the round after its first receipt) has
 * receipt round s + d(u, v).  The delay belongs to the unordered pair and is
 * fixed for the run: a link is as slow one way as the other, the same for every
 * message and row width, and parallel arcs of a raw CSR share it.  dmax = 1 is
 * the flood, bit for bit.  `sends`, `active` and GP_FORWARDS count attempted
 * sends in the send round.  A line already sent still arrives if its sender
 * crashes later; a receiver down in the arrival round loses it for good;
 * heartbeats are not delayed.  With gp_link_loss as well, the line sent in
 * round s arrives iff arc u -> v was open in round s.  Without loss and
 * liveness first[v][k] = inject[k] + the shortest-path distance from origin[k]
 * to v under d, and coverage equals the flood's.  A message table run in blocks
 * (msg_word_base) gives the columns of the whole run, and no gp_config tuning
 * field changes an output.
 *
 * Termination: a run is over after the first round r >= the last inject round
 * with new_bits = 0 and no sender in any round of [r + 2 - dmax, r] -- nothing
 * is in flight.  gp_run stops by this rule; a caller stepping gp_round reads
 * in_flight from gp_link_delay_info: the number of rounds s in
 * [round + 1 - dmax, round - 1] with active > 0 (0 with delay off).  Rounds
 * with new_bits = 0 occur before the end.
 *
 * gp_link_delay sets the request for the next gp_reset (on = 0: off; seed is
 * then ignored).  GP_EINVAL for dmax outside [1, 8], also with on = 0: the
 * previous request stays.  gp_link_delay_info reports the setting in force for
 * the current run (any pointer may be null).  GP_ARC_DELAY reads d per arc of
 * the in-CSR while delay is in force (GP_ENOTRACK otherwise).
 *
 * gp_reset fails with GP_EINVAL, and changes nothing, when delay is requested
 * together with gp_track_load, gp_track_fresh, gp_track_fresh_curve,
 * gp_track_link_fresh, gp_track_mult or gp_watch (they take every line to
 * arrive in its send round; gp_last_error names the record), in a
 * vertex-partitioned context, in a message-shard job (gp_shard_*), or on more
 * than 2^28 vertices; with GP_ENOMEM when the ring of dmax + 1 frontier-row
 * buffers cannot be allocated (no delay is then in force, gp_link_delay_info
 * says so, and the context stays usable: the request stands for the next
 * gp_reset, or is withdrawn).  A shard transport joined after the reset of a
 * delayed run makes every further gp_round fail with GP_ESTATE, before
 * anything of the round is enqueued.  gp_track_curve, gp_track_delay, gp_track_delay_dist,
 * track_first, track_digest, track_msg_forwards, coverage and forwards stay
 * exact.  Delayed rounds report gp_round_stats.mode = 2 and scan = 0.
 *
 * Checkpoints: the lines in flight are not in the blob.  gp_checkpoint_save
 * with dmax > 1 in force, and gp_checkpoint_load with dmax > 1 requested, fail
 * with GP_ESTATE; dmax = 1 behaves as gp_link_loss does. */
int gp_link_delay(gp_ctx* ctx, int32_t on, int32_t dmax, uint64_t seed);
int gp_link_delay_info(gp_ctx* ctx, int32_t* on, int32_t* dmax, uint64_t* seed, int32_t* in_flight);

/* Anti-entropy repair (csrc/repair.hip, csrc/repair_draw.h; DESIGN.md §2.2,
 * §2.6, §3.21).  Over lossy links a dropped line is lost for good.  With repair
 * on, round r is a repair round iff (r + 1) % period == 0, period in [1, 64],
 * and in one every up vertex v with an in-neighbour reconciles its whole
 * Message-List with one of them:
 *
 *   p_r(v) = col[row_ptr[v] + below(draw(stream_key(seed, 0x400 + r), (uint64_t)v), deg_in(v))]
 *
 * v a global vertex id, the in-CSR as loaded or built (GP_ROW_PTR / GP_COL).
 * The exchange happens iff p_r(v) is up in round r and arc p_r(v) -> v is open
 * in round r (gp_link_loss's draw: always with loss off, never at p = 1; the
 * exchange and the gossip line on the same arc in the same round share their
 * fate).  It offers v the messages p_r(v) held before this round's receipts
 * and v did not; they join the round's gossip: first receipts of receipt round
 * r + 1 like any other, with a first byte and a digest term, and v forwards
 * them once in round r + 1 -- repair restarts the flood.  `sends`, `active`
 * and GP_FORWARDS need no new rule.  A self-loop partner offers nothing, a
 * removed or crashed partner answers nothing, heartbeats are untouched.  The
 * partner draw sees the receiver and the round only: a message table run in
 * blocks (msg_word_base) gives the columns of the whole run, and no gp_config
 * tuning field changes an output.  Without loss (or with p = 0) repair changes
 * no first receipt: every message an up neighbour holds was sent to v in the
 * round after that neighbour first held it.
 *
 * Termination: the run is over after the first round r whose last `period`
 * rounds all lie at or after the last inject round and all have new_bits = 0
 * (period 1: the flood's rule).  gp_run stops by this rule; a caller stepping
 * gp_round reads `quiet` from gp_repair_info: the number of most recent
 * consecutive rounds at or after the last inject round with new_bits = 0.
 * With one random partner a silent period is NOT convergence: another draw
 * could still repair something.  It is only the stopping rule.  The 254-round
 * ceiling and its GP_ESTATE stay.
 *
 * gp_repair sets the request for the next gp_reset (on = 0: off; seed is then
 * ignored).  GP_EINVAL for a period outside [1, 64], also with on = 0: the
 * previous request stays.  gp_repair_info reports the setting in force for the
 * current run (any pointer may be null).  gp_read_repair writes, for each round
 * run since gp_reset (at most cap of them; *rounds gets their number), two
 * exact counts: out[r][0] = exchanges that happened in round r, out[r][1] =
 * the Message-List entries they carried (a bit gossip also delivered in that
 * round counts).  Both are 0 in a non-repair round.  Over the blocks of a
 * message table the lines add up and the exchanges are each block's own.
 * GP_ENOTRACK with repair off, GP_ESTATE for a run restored from a checkpoint
 * past round 0.
 *
 * gp_reset fails with GP_EINVAL, and changes nothing, when repair is requested
 * together with gp_link_delay, with gp_track_load, gp_track_fresh,
 * gp_track_fresh_curve, gp_track_link_fresh, gp_track_mult or gp_watch (with
 * or without loss; gp_last_error names the record), in a vertex-partitioned
 * context or in a message-shard job (gp_shard_*).  A shard transport joined
 * after the reset makes every further gp_round fail with GP_ESTATE, before
 * anything of the round is enqueued.  gp_track_curve, gp_track_delay,
 * gp_track_delay_dist, track_first, track_digest, track_msg_forwards, coverage
 * and forwards stay exact.  Every round of such a run reports
 * gp_round_stats.mode = 2 and scan = 0, and the context keeps the exact
 * frontier rows, as under gp_link_loss.
 *
 * Checkpoints: as for gp_link_loss.  The setting is not in the blob and the
 * draw depends on the round alone; only the repair record is lost, and `quiet`
 * restarts at 0. */
int gp_repair(gp_ctx* ctx, int32_t on, int32_t period, uint64_t seed);
int gp_repair_info(gp_ctx* ctx, int32_t* on, int32_t* period, uint64_t* seed, int32_t* quiet);
int gp_read_repair(gp_ctx* ctx, uint64_t* out /* [cap][2] */, int32_t cap, int32_t* rounds);

/* Checkpoints (no reference counterpart -- the
 * reference's peers keep no state across restarts).  Taken between rounds:
 * the blob holds the whole per-run state of this context (Message-List rows in
 * canonical form, popcounts, liveness state, counters, tracked outputs, round
 * number and direction history).  Loading it into a context with the same
 * overlay, messages, partition and tracked outputs continues the run exactly
 * as if it had never stopped.  The blob is opaque; gp_checkpoint_size gives
 * its length (8*W bytes per vertex plus ~30 B of vertex state). */
int gp_checkpoint_size(gp_ctx* ctx, int64_t* bytes);
int gp_checkpoint_save(gp_ctx* ctx, void* host, int64_t bytes);
int gp_checkpoint_load(gp_ctx* ctx, const void* host, int64_t bytes);

/* Self-test of the in-register lane operations the pull kernels reduce with
 * (csrc/lane_ops.h): sums, xors and ORs over the wave, over aligned groups of
 * 4 / 8 / 16 / 32 lanes and over the row slots of every row width.  One small
 * kernel on `device` evaluates each of the GP_LANE_SELFTEST_OPS operations
 * beside its LDS-shuffle form on the same data: 4 waves of 68 patterns (all
 * zero, all ones, each single lane set, the lane index, random words drawn
 * from `seed`).  out_mismatches holds 2 * GP_LANE_SELFTEST_OPS words:
 * [k] the lanes in which operation k's two forms differ (0 expected), and
 * [GP_LANE_SELFTEST_OPS + k] the sum, modulo 2^64, of the in-register form's
 * results over every pattern, wave and lane (for a check on the host).
 * Operations: 5 * kind + size, kind = u32 sum, u64 sum, u64 xor, u64 OR,
 * bool OR, size = groups of 4, 8, 16, 32 lanes, whole wave; then 25 .. 28 the
 * slot OR of rows of 64, 32, 16, 8 words, and 29 .. 31 the packed gather's
 * slot OR at 32, 16 and 8 lanes per slot.  Needs no context; no engine call
 * uses it. */
#define GP_LANE_SELFTEST_OPS 32
int gp_selftest_lane_ops(int device, uint64_t seed, uint64_t* out_mismatches);

#ifdef __cplusplus
}
#endif

#endif /* GOSSIP_CAPI_H */
