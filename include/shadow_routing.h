/*
 * shadow_routing.h — C ABI of the MI355X routing-table builder for Shadow.
 *
 * Drop-in boundary for ONE reference path: Shadow's all-pairs routing-table build
 *   NetworkGraph::compute_shortest_paths(&self, nodes: &[NodeIndex])
 *       -> Result<HashMap<(NodeIndex, NodeIndex), PathProperties>, NetGraphError>
 *   (/root/reference/src/main/network/graph/mod.rs:183-228)
 * and its use_shortest_path=false sibling
 *   NetworkGraph::get_direct_paths  (mod.rs:230-252, get_edge_weight mod.rs:254-293)
 * plus the ingest step in front of it
 *   NetworkGraph::parse              (mod.rs:134-181, gml-parser/src/parser.rs:44-281,
 *                                     ShadowNode/ShadowEdge mod.rs:28-111, units.rs:377-439)
 *
 * Plain C types only (no torch, no C++ types).  Every function is noexcept: errors are
 * integer status codes plus a message written to a caller buffer, formatted like the
 * reference's error strings so the Rust wrapper can forward them verbatim.
 *
 * Output layout: dense row-major num_nodes x num_nodes, indexed by POSITION in `nodes`
 * (out[i*num_nodes + j] = path nodes[i] -> nodes[j]).  The reference returns a HashMap
 * keyed by (NodeIndex, NodeIndex); the Rust-side binding in INTEGRATION.md rebuilds that
 * map (or, per SURVEY f1, keeps the dense arrays).  PathProperties is split SoA:
 * latency_ns (u64) + packet_loss (f32), because the Rust struct is not repr(C).
 */
#ifndef SHADOW_ROUTING_H
#define SHADOW_ROUTING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------- */
#define SRG_OK 0
#define SRG_ERR_ARG 1           /* bad argument (null pointer, index out of range, duplicate node) */
#define SRG_ERR_NO_EDGE 2       /* "No edge connecting node {src_id} to {dst_id}"       mod.rs:266-268 */
#define SRG_ERR_MULTI_EDGE 3    /* "More than one edge connecting node {a} to {b}"      mod.rs:269-274 */
#define SRG_ERR_UNREACHABLE 4   /* assert_eq!(paths.len(), nodes.len().pow(2)) panics   mod.rs:219 */
#define SRG_ERR_LATENCY_RANGE 5 /* latency.convert(Nano).unwrap() overflow (mod.rs:336), or a used
                                   pair with no path below 2^62 units on a graph whose worst-case
                                   path sum reaches 2^62 units (unit = srg_stats.latency_unit_ns, the
                                   gcd of the non-self-loop latencies).  The u64 keys hold distances
                                   below 2^62 units only (an edge of >= 2^62 units counts as absent),
                                   so such a pair may be unreachable OR have a shortest path in
                                   [2^62, 2^64) ns that the reference would return (e.g. one edge of
                                   2^63 + 1 ns) -- a documented deviation; a graph whose used pairs
                                   all have paths below 2^62 units succeeds whatever its latencies */
#define SRG_ERR_HIP 6           /* HIP runtime failure (no device, launch failure) */
#define SRG_ERR_OOM 7           /* device allocation failed */
#define SRG_ERR_PARSE 8         /* GML / attribute error from NetworkGraph::parse (mod.rs:134-181) */
#define SRG_ERR_RCCL 9          /* collective failure (multi-GPU) */
#define SRG_ERR_INTERNAL 10     /* invariant violated inside the builder (a bug) */

/* ---- graph as the Rust side would marshal it from petgraph ------------------------- */
/* One entry per petgraph edge, in graph.raw_edges() order (== GML edge order).
 * src/dst are NodeIndex values (dense 0..num_vertices-1, GML node order, mod.rs:157-162).
 * Self-loops and parallel edges are allowed exactly as in the reference.                */
typedef struct srg_edge_list {
    uint32_t num_vertices;
    uint32_t directed;          /* 1 = petgraph::Directed, 0 = Undirected (GML default 0) */
    uint64_t num_edges;
    const uint32_t* src;        /* [num_edges] */
    const uint32_t* dst;        /* [num_edges] */
    const uint64_t* latency_ns; /* [num_edges] latency.convert(Nano) (mod.rs:336) */
    const float* packet_loss;   /* [num_edges] raw f32 in [0,1] (mod.rs:95-103) */
    const uint32_t* node_ids;   /* [num_vertices] GML id per NodeIndex, for error text; may be NULL */
} srg_edge_list;

/* Timing / path report for one call (all fields written when the pointer is non-NULL). */
typedef struct srg_stats {
    double ms_total;            /* entry -> return wall time */
    double ms_h2d;              /* host -> device copies (host entry points only) */
    double ms_build;            /* dense weight-matrix build + validation kernels */
    double ms_fw;               /* blocked Floyd-Warshall (dense) / batched Bellman-Ford (sparse) */
    double ms_scan;             /* essential-edge extraction + tight-predecessor scan */
    double ms_loss;             /* left-fold loss rounds over the tight DAG */
    double ms_extract;          /* used x used sub-matrix + diagonal self-loop overwrite */
    double ms_d2h;              /* device -> host copies (host entry points only) */
    int32_t path_kind;          /* SRG_PATH_* below */
    int32_t loss_rounds;        /* max fold rounds over rows (DAG depth + 1) */
    uint64_t multi_pred_pairs;  /* (s,t) pairs with >1 tight predecessor (slow path); u64 keys: the pairs whose
                                 * keys' low words tie, which the loss pass decides exactly (an upper bound) */
    uint64_t relaxations;       /* min-plus relaxations issued by the FW kernels */
    uint64_t essential_edges;   /* edges with W[u][t] == D[u][t] (candidates for tightness) */
    int32_t scan_kind;          /* SRG_SCAN_* below */
    int32_t table_keys;         /* srg_routing_info_build: 1 = the table kept the build's u32 latency keys
                                   (latency = key x latency_unit_ns; 0.4 GB less D2H and host memory at C3),
                                   0 = u64 ns (u64-key builds, several ranks, direct paths) */
    /* filled only when profiling is enabled (SRG_OPT_PROFILING): HIP events recorded on the
     * launch stream around every launch of the dominant kernel (FW phase-3 product).      */
    uint64_t prof_launches;     /* profiled launches */
    double prof_kernel_ms;      /* sum of their event-measured durations */
    uint64_t prof_relaxations;  /* relaxations those launches performed */
    /* multi-rank (srg_comm_init*): this rank's view */
    double ms_exchange;         /* output row exchange (all ranks end with every row) */
    int32_t nranks;             /* ranks in the communicator (1 = single GPU) */
    int32_t rank;               /* this rank */
    uint64_t local_sources;     /* used sources routed by this rank */
    /* host entry: the caller's output arrays are page-locked concurrently with H2D + FW, then
     * finished rows leave while later kernels run; ms_d2h above is only the exposed tail.   */
    double ms_host_register;    /* page-locking time (hidden; -1 = not used / failed)      */
    uint64_t d2h_overlapped_bytes; /* output bytes copied to the host while kernels ran    */
    uint64_t min_latency_ns;    /* host entry: min latency over all n^2 outputs, diagonal included
                                   (RoutingInfo::get_smallest_latency_ns, mod.rs:474-476);
                                   UINT64_MAX when n = 0                                       */
    uint64_t latency_unit_ns;   /* shortest paths: the gcd of the non-self-loop edge latencies; the
                                   kernels count latency in these units (exact: every path sum is a
                                   multiple), outputs are back in ns.  1 = nanosecond keys        */
    int32_t fw_overlap_pivots;  /* host entry: FW pivots enqueued while the edge list was still crossing
                                   PCIe (SRG_OPT_FW_OVERLAP; 0 = none)                              */
    int32_t fw_overlap_kept;    /* host entry: 1 = the FW that ran beside the H2D produced the table
                                   (its certification passed), 0 = the build ran FW after the H2D   */
    int32_t d2h_key_rows;       /* host entry, u64 output: 1 = the latency rows crossed PCIe as the build's
                                   u32 keys (4 B instead of 8 per pair) and were widened on the host  */
    int32_t reserved0;
    double ms_key_widen;        /* its widening + key-copy wall time on the helper thread (overlapped
                                   with the loss pass; the part after the kernels is in ms_d2h)     */
} srg_stats;

#define SRG_PATH_DENSE_U32 0    /* dense FW, u32 saturating latency keys (exact, certified) */
#define SRG_PATH_DENSE_U64 1    /* dense FW, u64 latency keys */
#define SRG_PATH_DIRECT 2       /* get_direct_paths */
#define SRG_PATH_SPARSE_U32 3   /* sparse: batched lexicographic Bellman-Ford, u32 latency keys */
#define SRG_PATH_SPARSE_U64 4   /* sparse, u64 latency keys (used paths past 2^32-1 latency units) */

#define SRG_SCAN_NONE 0         /* no used sources */
#define SRG_SCAN_SPARSE 1       /* tight scan over the essential edges (default) */
#define SRG_SCAN_DENSE 2        /* tight scan over all (s,u,t) triples (essential-dense graphs) */

typedef struct srg_ctx srg_ctx; /* opaque: owns device workspace; one HIP device */

/* Create a context bound to HIP device `device` (one process per GPU).  Besides the HIP runtime's
 * device initialisation it warms what the first host-entry call would otherwise pay on the routing
 * path: the kernels' code object on the device, each stream's first dispatch, the H2D codec's worker
 * pool and page-locked rings, the first H2D / D2H / SDMA copies (SRG_CREATE_WARM=0 in the environment
 * skips that, for A/B).  Shadow creates its context before parsing the GML, so this
 * runs off the routing path.  Replaces nothing in the reference: the context is the device state that
 * compute_shortest_paths (mod.rs:183-228) needs and Rust's CPU path does not have. */
int srg_create(srg_ctx** out, int device, char* errbuf, size_t errlen);
void srg_destroy(srg_ctx* ctx);


/* Context options.
 *   SRG_OPT_PROFILING         1 = HIP-event timing of every dominant-kernel launch (stats.prof_*)
 *   SRG_OPT_SPARSE_THRESHOLD  essential-edge density (E_ess / V^2) up to which the sparse
 *                             tight scan is used (default 0.35; 0 forces the dense scan)      */
#define SRG_OPT_PROFILING 1
#define SRG_OPT_SPARSE_THRESHOLD 2
#define SRG_OPT_GATHER_OUTPUT 3   /* multi-rank: 1 (default) = every rank ends with all rows;
                                     0 = each rank fills only the rows of the sources it owns (the host
                                     entry then copies only those rows to the caller, and
                                     stats.min_latency_ns is over those rows) */
#define SRG_OPT_ALGORITHM 4       /* SRG_ALGO_*: how compute_shortest_paths routes */
#define SRG_ALGO_AUTO 0           /* sparse when V >= 2048 and arcs * 32 < V^2, else dense */
#define SRG_ALGO_DENSE 1          /* blocked FW + tight-DAG loss pass */
#define SRG_ALGO_SPARSE 2         /* batched lexicographic Bellman-Ford over CSR */
#define SRG_OPT_SPARSE_LOCALITY 5 /* sparse: 1 (default) = batch sources in BFS order, 0 = in `nodes` order */
#define SRG_OPT_SIMULATE_RANK 6   /* TIMING AID ONLY: value = nranks*1000 + rank runs this rank's share
                                     with every collective elided -- outputs are NOT valid; 0 detaches */
#define SRG_OPT_FW_TILE 7         /* dense u32 FW tile: 0 = auto (128), 64, 128 */
/* 8 (SRG_OPT_FW_PACKED) and 18 (SRG_OPT_CHAIN_PRIO) were A/B switches, removed in round 4: the u32 FW
 * always runs the pair-packed tile and the chain kernels always raise their priority. */
/* 10 (SPARSE_GROUP), 11 (SPARSE_WGS_PER_CU) and 13 (SPARSE_DELTA_ALL) were A/B switches of the sparse
 * kernel, removed in round 4: 8 rows in flight, two workgroups per CU, any-lane bucket test. */
#define SRG_OPT_SPARSE_DELTA_DIV 12  /* sparse: delta-stepping bucket width = max edge latency / value;
                                        0 = a single bucket (plain Bellman-Ford); default 1 */
#define SRG_OPT_SPARSE_GLOBAL_BITMAPS 14 /* sparse: 1 = keep the per-batch vertex bitmaps in global memory
                                        (automatic when 5V/8 bytes do not fit the LDS budget) */
#define SRG_OPT_FW_SYMMETRIC 17     /* dense: 1 (default) = for an undirected graph, update only the FW tiles
                                       I <= J (D stays symmetric; u32 keys on 128-tiles, u64 keys on 64-tiles,
                                       one rank or many) and mirror at the end; 0 = the general FW */
#define SRG_OPT_D2H_MODE 20         /* host entry: how finished rows are shipped into the page-locked caller
                                     * arrays while kernels run: 1 (default) = an SDMA engine, 0 =
                                     * hipMemcpyAsync (a full-chip blit kernel: slows the overlapped kernels) */
#define SRG_OPT_LOSS_CHUNKS 21       /* dense: k_loss_rows launches (row chunks); 0 (default) = 8 when the host
                                     * entry ships rows early, else 1 */
#define SRG_OPT_SCAN_GROUPS 22       /* host entry: source-block groups the tight scan is
                                     * launched in, each group's loss rows folded and shipped while
                                     * later groups scan; 0 (default) = 3 (4 when the scan is mirrored,
                                     * SRG_OPT_SCAN_MIRROR), 1 = scan, then loss */
#define SRG_OPT_H2D_CODEC 25         /* host entry: 1 (default) = the edge list crosses PCIe narrowed (u16
                                     * endpoints, u32 latencies; 12 instead of 20 B per edge) when every
                                     * endpoint < 65536 and latency < 2^32, widened on the device; 0 = plain */
#define SRG_OPT_EDGE_SHARD 29        /* host entry, multi-rank: 1 = each rank ships 1/N of the edge list over
                                     * its own PCIe link and the ranks exchange the slices over the GPU
                                     * links (allgatherv); 0 = every rank ships the whole list; -1 (default)
                                     * = 1 when the group has >= 4 ranks */
#define SRG_OPT_LATE_LOSS 30         /* host entry: 1 (default) = the edge losses cross PCIe after the endpoints
                                     * and latencies, on their own stream beside the W build and FW (which
                                     * need no loss); 0 = with them */
#define SRG_OPT_FW_LINE_SPLIT 31     /* symmetric FW: sub-tiles per dimension of the critical chain's line
                                     * launches, 1 (whole 128-tiles) / 2 / 4; 0 (default) = by the bulk a
                                     * pivot leaves this rank: >= 2048 tiles 1, >= 1024 tiles 2, else 4
                                     * (C3: 1 on one rank, 2 on two, 4 on more; C1/C2: 4) */
#define SRG_OPT_FW_STEP 32           /* symmetric FW schedule.  -1 (default) = the bulk and the next pivot's chain
                                     * on two streams; between ranks the chain exchanges its line segments
                                     * device-side (stores into the peers' line buffers + arrival words) for
                                     * simulated ranks and in-process ranks on distinct devices, else with
                                     * the communicator's allgather.  0 = two streams, always the allgather.
                                     * 2 = two streams, device-side exchange also for ranks sharing a GPU
                                     * (each rank's chain stream needs a hardware queue of its own).
                                     * 1 = one fused launch per pivot (chain on the launch's first
                                     * workgroups, exchange inside it; measured slower) */
#define SRG_OPT_FW_OVERLAP 33        /* host entry, one rank: 1 (default) = FW starts while the edge list is still
                                     * crossing PCIe (an undirected list ordered by source row with every edge
                                     * (s, d), s <= d -- a GML complete graph: each block-row of W is split and
                                     * caught up on the pivots already run as soon as its edges have landed);
                                     * 0 = FW after the whole list (any list falls back to that by itself) */
#define SRG_OPT_TEST_FAULT 34         /* TEST BUILD ONLY: compiled in only with -DSRG_TEST_HOOKS (the test library
                                     * libshadow_routing_testhooks.so); the product library refuses any value
                                     * but 0 with SRG_ERR_ARG.  1 = overwrite the closed FW matrix
                                     * with zeros after FW (a lost synchronisation's result: the build must fail
                                     * with SRG_ERR_INTERNAL, not return it); 2 = nonzero FW sync words and zero
                                     * line buffers before each symmetric FW (a recycled allocation: the build
                                     * must still be exact); 0 (default) = off */
#define SRG_OPT_TABLE_POOL_BYTES 35  /* RoutingInfo tables (srg_routing_info_build, one rank) come from a pool of
                                     * page-locked host tables on the context; freeing a RoutingInfo returns
                                     * them, so the next build skips the prefault + page-locking.  Bytes of idle
                                     * tables the pool keeps (default: no byte cap, only the most recently freed
                                     * table pair; setting a byte cap replaces that count cap; 0 = free them at
                                     * once).  Idle tables stay page-locked (not reclaimable by the OS) until
                                     * reused, trimmed or srg_destroy */
#define SRG_OPT_TABLE_POOL_IDLE_BYTES 36  /* read-only: bytes of idle tables the pool holds now */
#define SRG_OPT_CREATE_MS_RUNTIME 37  /* read-only: srg_create's HIP-runtime part (device count, device context,
                                      * the first stream, where the runtime initialises the device: the first
                                      * context of a process pays the runtime's initialisation) */
#define SRG_OPT_CREATE_MS_LIBRARY 38  /* read-only: srg_create's own part (three more streams, mailbox, SDMA
                                      * agents, events, the warm-up) */
#define SRG_OPT_FW_XCD_ORDER 39      /* symmetric FW bulk launch order: 1 (default) = the tiles dealt to the 8 XCDs as
                                     * Z-order runs, one list per pivot (each XCD a compact block of the triangle,
                                     * its line-buffer operands L2-resident: C3 bulk HBM traffic 1.38x -> 1.12x of
                                     * the C tiles); 0 = triangle order (consecutive tiles round-robin) */
#define SRG_OPT_SCAN_MIRROR 40       /* dense build, sparse tight scan: 1 (default) = on an undirected graph whose
                                     * used nodes are all vertices in order (one rank, u32 keys) scan only the
                                     * (source block, target tile) pairs on and above the diagonal and derive
                                     * the pairs below it from them; 0 = scan every pair.  Every
                                     * other build scans every pair */
#define SRG_OPT_SCAN_MIRRORED 41     /* read-only: the last build's scan: 0 = every pair scanned, 1 = mirrored,
                                     * 2 = mirrored, then scanned again in full (its worklist overflowed) */
#define SRG_OPT_SCAN_MIRROR_CAP 42   /* pairs the mirror's exact-key worklist holds per launch; 0 (default) =
                                     * 1 / 1024 of the launch's pairs (at least 256); at most what the packed
                                     * predecessor rows leave free (half the launch's pairs) */
#define SRG_OPT_LOSS_KIND 43         /* read-only: the last dense build's loss pass: 0 = none (no dense build, or
                                     * no local source), 1 = per-row fold in LDS (k_loss_rows), 2 = global-memory
                                     * fold over the essential entries (k_loss_round_sparse: rows too long for
                                     * LDS), 3 = dense-scan fold (k_loss_round).  The tests read it to prove which
                                     * pass they ran; the limits that select it (the list's LM_T x LM_E, the
                                     * mirror's step limit, the largest V of the LDS fold) come from
                                     * srg_internal_loss_limits (csrc/internal.h), and the environment switch
                                     * SRG_LOSS_ROWS_MAX_V (csrc/env_switches.h) lowers the last one */
#define SRG_OPT_ROUTE_TREE_ROWS 44   /* source rows per batch of srg_route_trees_device and
                                     * srg_link_loads_trees_device; 0 (default) = as many as a fixed workspace
                                     * budget of 4 GiB allows (the bytes per row are listed with the two calls) */
#define SRG_LOSS_NONE 0
#define SRG_LOSS_ROWS_LDS 1
#define SRG_LOSS_GLOBAL_ENTRIES 2
#define SRG_LOSS_DENSE_SCAN 3
int srg_set_option(srg_ctx* ctx, int option, double value);
/* current value of an option (SRG_OK), or SRG_ERR_ARG for an unknown option */
int srg_get_option(srg_ctx* ctx, int option, double* value);

/* Replaces NetworkGraph::compute_shortest_paths (mod.rs:183-228).
 * Host pointers in, host pointers out.  out_* are caller-allocated num_nodes^2.
 * Diagonal = raw self-loop weight (mod.rs:210-217); errors in `nodes` order.           */
int srg_compute_shortest_paths(srg_ctx* ctx, const srg_edge_list* graph,
                               const uint32_t* nodes, uint32_t num_nodes,
                               uint64_t* out_latency_ns, float* out_packet_loss,
                               srg_stats* stats, char* errbuf, size_t errlen);

/* Same computation with every array already resident in device memory (HBM):
 * graph->src/dst/latency_ns/packet_loss/node_ids, nodes and out_* are device pointers;
 * `hip_stream` is a hipStream_t (NULL = default stream).  Returns after the stream work
 * is complete.  (The benchmark's headline times the HOST entry above, as Shadow calls it;
 * this entry is reported beside it as the inputs-resident-in-HBM figure.)              */
int srg_compute_shortest_paths_device(srg_ctx* ctx, const srg_edge_list* graph_dev,
                                      const uint32_t* nodes_dev, uint32_t num_nodes,
                                      uint64_t* out_latency_ns_dev, float* out_packet_loss_dev,
                                      void* hip_stream, srg_stats* stats,
                                      char* errbuf, size_t errlen);

/* Replaces NetworkGraph::get_direct_paths (mod.rs:230-252): every used pair <- the single
 * edge src->dst (undirected: either orientation), error unless exactly one exists.     */
int srg_get_direct_paths(srg_ctx* ctx, const srg_edge_list* graph,
                         const uint32_t* nodes, uint32_t num_nodes,
                         uint64_t* out_latency_ns, float* out_packet_loss,
                         srg_stats* stats, char* errbuf, size_t errlen);

/* ---- RoutingInfo, dense-backed ------------------------------------------
 * Replaces generate_routing_info (src/main/core/sim_config.rs:425-462) and RoutingInfo<u32>
 * (mod.rs:428-477).  The reference builds two n^2-entry HashMaps (mod.rs:190-208 and
 * sim_config.rs:448-450); here the table is the dense n x n SoA the GPU wrote plus a GML-id ->
 * position index, so building it costs one host-entry call (srg_compute_shortest_paths).     */
typedef struct srg_routing_info srg_routing_info;
/* gml_ids[num_ids]: the used nodes' GML ids (ip_assignment.get_nodes(), any order); they are
 * resolved with graph->node_ids (node_id_to_index, mod.rs:126-128; NULL = id == index).
 * use_shortest_paths = network.use_shortest_path (configuration.rs:286-292).  Errors carry the
 * reference's context prefix ("Failed to compute shortest paths between graph nodes: ...").   */
int srg_routing_info_build(srg_ctx* ctx, const srg_edge_list* graph, const uint32_t* gml_ids, uint32_t num_ids,
                           int use_shortest_paths, srg_routing_info** out, srg_stats* stats,
                           char* errbuf, size_t errlen);
/* The same, built by every GPU of an srg_multi (declared below). */
struct srg_multi;
int srg_routing_info_build_multi(struct srg_multi* m, const srg_edge_list* graph, const uint32_t* gml_ids,
                                 uint32_t num_ids, int use_shortest_paths, srg_routing_info** out, srg_stats* stats,
                                 char* errbuf, size_t errlen);
void srg_routing_info_free(srg_routing_info* ri);
uint32_t srg_routing_info_num_nodes(const srg_routing_info* ri);
/* RoutingInfo::path (mod.rs:444-446): 1 and the path's properties, or 0 (None).              */
int srg_routing_info_path(const srg_routing_info* ri, uint32_t start_id, uint32_t end_id,
                          uint64_t* latency_ns, float* packet_loss);
/* RoutingInfo::increment_packet_count (mod.rs:449-456): saturating, thread-safe.              */
void srg_routing_info_increment_packet_count(srg_routing_info* ri, uint32_t start_id, uint32_t end_id);
uint64_t srg_routing_info_packet_count(srg_routing_info* ri, uint32_t start_id, uint32_t end_id);
/* RoutingInfo::get_smallest_latency_ns (mod.rs:474-476): 1 and the min over all entries
 * (diagonal included), or 0 (None, empty table).                                               */
int srg_routing_info_smallest_latency_ns(const srg_routing_info* ri, uint64_t* out);
/* Borrowed dense tables (row-major by position) and the GML id of each position.             */
void srg_routing_info_tables(const srg_routing_info* ri, const uint64_t** latency_ns, const float** packet_loss,
                             const uint32_t** gml_ids, uint32_t* n);

/* ---- ingest: GML text -> graph (NetworkGraph::parse, mod.rs:134-181) --------------- */
typedef struct srg_graph srg_graph;  /* opaque host-side parsed graph */

int srg_graph_parse_gml(const char* text, size_t len, srg_graph** out,
                        char* errbuf, size_t errlen);
void srg_graph_free(srg_graph* g);
/* Borrowed view of the edge list (valid until srg_graph_free). */
void srg_graph_edge_list(const srg_graph* g, srg_edge_list* out);
uint32_t srg_graph_num_vertices(const srg_graph* g);
uint64_t srg_graph_num_edges(const srg_graph* g);
int srg_graph_directed(const srg_graph* g);
/* node_id_to_index (mod.rs:126-128): SRG_OK or SRG_ERR_ARG if the id is unknown. */
int srg_graph_node_index(const srg_graph* g, uint32_t gml_id, uint32_t* out_index);
/* node_index_to_id (mod.rs:130-132). */
uint32_t srg_graph_node_id(const srg_graph* g, uint32_t index);
/* ShadowNode bandwidths in bit/s (mod.rs:34-57); has_* = 0 when the key was absent.   */
void srg_graph_node_bandwidth(const srg_graph* g, uint32_t index,
                              uint64_t* down_bits, int* has_down,
                              uint64_t* up_bits, int* has_up);
/* All nodes at once: arrays of srg_graph_num_vertices entries (any pointer may be NULL).      */
void srg_graph_node_bandwidths(const srg_graph* g, uint64_t* down_bits, int* has_down,
                               uint64_t* up_bits, int* has_up);
/* Diagnostics: how many text chunks the last parse of `g` used (1 = one sequential pass).    */
uint32_t srg_graph_parse_chunks(const srg_graph* g);

/* ---- multi-GPU: one process (or thread) per GPU, SPMD -------------------------------
 * After srg_comm_init*, every rank calls srg_compute_shortest_paths[_device] with the SAME
 * graph and nodes.  Undirected graphs: the symmetric FW's stored tiles (I, J), I <= J, are dealt
 * to rank (I + J) mod G and each pivot's line buffer (the pivot's row panel = its column panel)
 * is exchanged once per pivot (allgather; SRG_OPT_FW_STEP = 2: device-side stores); directed
 * graphs: row blocks with a per-pivot broadcast of the row panel.  Each rank routes the used
 * sources at positions [n r / G, n (r+1) / G) of `nodes`; output rows are exchanged
 * (SRG_OPT_GATHER_OUTPUT).  The reference has no multi-process path (rayon threads only,
 * mod.rs:190-208): this is new, MI355X-side design.                         */
#define SRG_UNIQUE_ID_BYTES 128
/* RCCL (over xGMI): rank 0 creates the id, the caller shares it (e.g. torch.distributed). */
int srg_comm_unique_id(unsigned char id[SRG_UNIQUE_ID_BYTES], char* errbuf, size_t errlen);
int srg_comm_init(srg_ctx* ctx, int nranks, int rank, const unsigned char id[SRG_UNIQUE_ID_BYTES],
                  char* errbuf, size_t errlen);
/* In-process group: several contexts of ONE process (threads; may share one GPU). */
typedef struct srg_local_group srg_local_group;
int srg_local_group_create(int nranks, srg_local_group** out);
void srg_local_group_release(srg_local_group* g);
int srg_comm_init_local(srg_ctx* ctx, srg_local_group* g, int rank, char* errbuf, size_t errlen);
int srg_comm_size(srg_ctx* ctx, int* nranks, int* rank);

/* ---- several GPUs behind ONE call (Shadow's one-process model) ------------------------
 * Shadow builds RoutingInfo once, in one process (sim_config.rs:137-141 -> manager.rs:301-324),
 * so the drop-in for a multi-GPU node is one object driving N devices: one context per device in
 * an in-process group (collectives are pull kernels over xGMI, peer access enabled), one worker
 * thread per rank.  srg_multi_compute_shortest_paths has exactly srg_compute_shortest_paths'
 * arguments and results: the whole n x n table lands in the caller's two arrays, every GPU
 * shipping its own sources' rows over its own PCIe link.  stats: wall times of the slowest
 * rank, counts summed over ranks, nranks = N.  A device may be listed more than once (several
 * ranks sharing one GPU: how the one-GPU test box exercises this path).                     */
typedef struct srg_multi srg_multi;
int srg_multi_create(srg_multi** out, const int* devices, int num_devices, char* errbuf, size_t errlen);
void srg_multi_destroy(srg_multi* m);
int srg_multi_size(const srg_multi* m);
/* srg_set_option on every rank (SRG_OPT_GATHER_OUTPUT and SRG_OPT_SIMULATE_RANK are fixed: ERR_ARG) */
int srg_multi_set_option(srg_multi* m, int option, double value);
int srg_multi_compute_shortest_paths(srg_multi* m, const srg_edge_list* graph, const uint32_t* nodes,
                                     uint32_t num_nodes, uint64_t* out_latency_ns, float* out_packet_loss,
                                     srg_stats* stats, char* errbuf, size_t errlen);
/* get_direct_paths (use_shortest_path = false) on the first device: an n^2 gather, no SSSP work */
int srg_multi_get_direct_paths(srg_multi* m, const srg_edge_list* graph, const uint32_t* nodes, uint32_t num_nodes,
                               uint64_t* out_latency_ns, float* out_packet_loss, srg_stats* stats, char* errbuf,
                               size_t errlen);

/* ---- stretch: one round's cross-host packet-event batch ---------------
 * Replaces, for a whole batch at once, the per-packet tail of Worker::send_packet
 * (src/main/core/worker.rs:391-424: latency lookup in RoutingInfo, deliver time raised to the
 * round end, lowest used latency for the dynamic runahead runahead.rs:61-116, next event time)
 * and the per-destination EventQueue ordering (worker.rs:644-654, event_queue.rs:38-49,
 * Event::partial_cmp event.rs:84-155: time, then src_host_id, then src_host_event_id), plus the
 * round's minimum next-event time (manager.rs:459-464).  The latency table is the dense
 * num_nodes x num_nodes output of srg_compute_shortest_paths (rows = sending node position).
 * Outputs: deliver_ns[i] per event; order = event indices grouped by destination host
 * (increasing HostId), each host's events in its queue's pop order; host_offsets[h] ..
 * host_offsets[h+1] = host h's slice.  This entry starts at the latency lookup: the packet-drop
 * decision (worker.rs:374-390) and increment_packet_count (:395) above it are covered by
 * srg_send_packets_device below, which takes the host-drawn `chance` values as an array.     */
#define SRG_ERR_EVENT_ORDER 11  /* two events with no relative order: PanickingOrd unwrap panic
                                   (event.rs:141-147, event_queue.rs:87-90) */
typedef struct srg_event_batch {
    uint64_t num_events;
    const uint32_t* src_node;      /* [n] row of the latency table (sender's node position)   */
    const uint32_t* dst_node;      /* [n] column of the latency table                          */
    const uint32_t* src_host;      /* [n] HostId of the sender                                 */
    const uint32_t* dst_host;      /* [n] HostId of the receiver, < num_hosts                  */
    const uint64_t* send_time_ns;  /* [n] Worker::current_time at the send (EmulatedTime ns)   */
    const uint64_t* src_event_id;  /* [n] src_host.get_new_event_id()                          */
    uint32_t num_hosts;
    uint32_t reserved;
    uint64_t round_end_ns;         /* Worker::round_end_time                                   */
} srg_event_batch;

typedef struct srg_event_result {
    uint64_t min_next_event_ns;    /* min deliver time (UINT64_MAX when empty)                 */
    uint64_t min_used_latency_ns;  /* min latency used (UINT64_MAX when empty)                 */
    uint32_t key_bits;             /* composite sort-key width actually used                   */
    uint32_t radix_passes;         /* 8-bit LSD passes run                                     */
    double ms_total;
} srg_event_result;

/* Device pointers throughout (batch arrays, table, outputs); `hip_stream` as above.          */
int srg_order_packet_events_device(srg_ctx* ctx, const srg_event_batch* batch_dev,
                                   const uint64_t* latency_table_dev, uint32_t table_n,
                                   uint64_t* out_deliver_ns_dev, uint32_t* out_order_dev,
                                   uint64_t* out_host_offsets_dev, void* hip_stream,
                                   srg_event_result* result, char* errbuf, size_t errlen);

/* ---- the whole per-packet tail of Worker::send_packet, batched --------------------------
 * srg_order_packet_events_device plus the lines above its start (worker.rs:374-395):
 *   reliability = 1.0f32 - packet_loss(src, dst), widened to f64      (worker.rs:563-568)
 *   dropped iff !is_bootstrapping && chance >= reliability && payload_size > 0   (:374-390)
 *   increment_packet_count(src, dst) for every packet sent             (:395, mod.rs:449-456)
 * against the table in either form a RoutingInfo keeps (u64 ns, or the build's u32 keys: no
 * widening, srg_routing_info_key_tables).  Only the RNG stays on the host: `chance` is
 * src_host.random_mut().gen::<f64>(), drawn unconditionally for every packet (worker.rs:377), so
 * the caller draws it per packet in program order and hands the array over.
 * Left to the caller, before an event enters the batch: the is_completed early return
 * (worker.rs:336-343) and the drop of a packet whose dst_ip resolves to no host (no dst_host to
 * give: dst_host >= num_hosts stays SRG_ERR_ARG).  Neither consumes a draw the batch could see.
 * Outputs: status[i] = 1 sent (PDS_INET_SENT) / 0 dropped (PDS_INET_DROPPED); deliver_ns[i], or
 * UINT64_MAX for a dropped event; order = the num_sent sent indices, grouped and ordered as above
 * (out_order_dev holds num_events slots, num_sent are written); host_offsets[num_hosts] = num_sent.
 * A dropped event takes no part in anything after its decision: the overflow check of send +
 * latency, the minima, the equal-key check (SRG_ERR_EVENT_ORDER), order and offsets.  The node and
 * dst_host range checks apply to every event.
 * packet_counts_dev (may be NULL): caller-owned [n*n] u64 by node position, NOT cleared --
 * accumulated across calls; [src_node, dst_node] += 1 per sent event, saturating at UINT64_MAX.
 * The counters move as soon as the range checks passed (also when the call then returns
 * SRG_ERR_EVENT_ORDER).  Merge them into a RoutingInfo with srg_routing_info_add_packet_counts. */
typedef struct srg_path_table_dev {   /* routing table resident in HBM, indexed by node position */
    uint32_t n, reserved;
    const uint64_t* latency_ns;   /* [n*n] u64 ns, or NULL when latency_key is given            */
    const uint32_t* latency_key;  /* [n*n] u32 keys: latency = key * unit_ns off the diagonal   */
    const uint64_t* diag_ns;      /* [n]   with latency_key: raw self-loop latency per position */
    uint64_t unit_ns;             /*       with latency_key                                     */
    const float* packet_loss;     /* [n*n]; NULL = no drop decision, every packet is sent       */
} srg_path_table_dev;

typedef struct srg_send_batch {
    srg_event_batch ev;           /* as srg_order_packet_events_device                          */
    const double* chance;         /* [n] host-drawn f64 in [0,1), program order (worker.rs:377) */
    const uint32_t* payload_size; /* [n] packet_getPayloadSize, only > 0 matters                */
    uint64_t bootstrap_end_ns;    /* sends before it are never dropped (worker.rs:337-338)      */
} srg_send_batch;

typedef struct srg_send_result { srg_event_result ev; uint64_t num_sent, num_dropped; } srg_send_result;

/* SRG_ERR_ARG unless exactly one of latency_ns / latency_key is given, diag_ns and unit_ns >= 1
 * come with latency_key, and chance and payload_size come with packet_loss.                    */
int srg_send_packets_device(srg_ctx* ctx, const srg_send_batch* batch_dev, const srg_path_table_dev* table,
                            uint8_t* out_status_dev, uint64_t* out_deliver_ns_dev, uint32_t* out_order_dev,
                            uint64_t* out_host_offsets_dev, uint64_t* packet_counts_dev /* may be NULL */,
                            void* hip_stream, srg_send_result* result, char* errbuf, size_t errlen);

/* A RoutingInfo whose table kept the build's u32 keys (srg_stats.table_keys = 1): returns 1 and
 * borrowed host views (key [n*n], diag_ns [n], unit_ns, packet_loss [n*n]) -- what
 * srg_path_table_dev takes, uploaded as they are.  Returns 0 for a u64 table (use
 * srg_routing_info_tables).  Never builds the u64 view that srg_routing_info_tables widens.     */
int srg_routing_info_key_tables(const srg_routing_info* ri, const uint32_t** key, const uint64_t** diag_ns,
                                uint64_t* unit_ns, const float** packet_loss, uint32_t* n);
/* Merges a batch counter table (packet_counts_dev copied to the host, n*n by position) into the
 * counters behind increment_packet_count / packet_count: every nonzero entry is saturating-added
 * under the GML ids of its positions.  Thread-safe against the per-packet calls.                */
void srg_routing_info_add_packet_counts(srg_routing_info* ri, const uint64_t* counts_by_position /* host, n*n */);

/* ---- device-resident per-host packet-event queues, across rounds ------------------------
 * The two batch entries above order one round's sends in isolation; these keep the per-host
 * EventQueues themselves (event_queue.rs:10-55) in HBM: a round's sent events are merged in at the
 * barrier, a window's events are popped out in the reference's order.  Packet events only: Local
 * events (and the CPU-delay re-push, host.rs:841-843) stay with the host, which interleaves its
 * popped packet slice with its local heap by (time, Packet before Local) (event.rs:103-110).
 *   one queue per destination host; total order (time, src_host_id, src_host_event_id)
 *   push of two events of one host equal in all three, one of them possibly resident:
 *        SRG_ERR_EVENT_ORDER
 *   push of an event with time < its host's last popped time (assert!, event_queue.rs:33):
 *        SRG_ERR_TIME_BACKWARD; time == last popped is accepted
 *   pop(until) removes, per host, exactly the events with time < until (Host::execute,
 *        host.rs:809-818) and sets the host's last popped time to the largest popped time
 *   min_next_event_ns after either call = the minimum head time over all hosts (UINT64_MAX when
 *        everything is empty): the manager's min_next_event_time (manager.rs:416-435, 459-464)
 * Any call that returns an error leaves the queues exactly as they were.  Both calls return after
 * their stream work is complete.  Cost: push O(backlog + batch) (a merge, never a re-sort); pop
 * O(popped + num_hosts), the kept backlog is not rewritten.                                     */
#define SRG_ERR_TIME_BACKWARD 12
/* opaque; lives in the HBM of ctx's device; not thread-safe; destroy it before its ctx */
typedef struct srg_event_queues srg_event_queues;
/* reserve_events: capacity allocated up front; growth past it reallocates geometrically and keeps
 * the contents (a failed allocation is SRG_ERR_OOM with the queues unchanged) */
int srg_event_queues_create(srg_ctx* ctx, uint32_t num_hosts, uint64_t reserve_events, srg_event_queues** out,
                            char* errbuf, size_t errlen);
void srg_event_queues_destroy(srg_event_queues* q);
/* merged outputs per merge workgroup (the tests place events around its multiples) */
uint32_t srg_event_queues_merge_tile(void);

typedef struct srg_queue_result {
    uint64_t num_moved;          /* pushed / popped by this call (pop: the count needed when capacity was short) */
    uint64_t num_queued;         /* live events after the call */
    uint64_t min_next_event_ns;  /* min head over hosts after the call */
    double ms_total;
} srg_queue_result;

/* batch_dev, deliver_ns_dev, order_dev[num_order]: exactly what srg_order_packet_events_device
 * (num_order = num_events) or srg_send_packets_device (num_order = num_sent) took and wrote.
 * tag_dev[num_events]: the caller's opaque u64 per event (the packet handle); NULL = the event's
 * index.  Validated on the device: order[i] < num_events, dst_host < the queues' num_hosts, and the
 * gathered keys strictly increase under (dst_host, time, src_host, event_id); otherwise
 * SRG_ERR_ARG ("order is not the batch's queue order").                                          */
int srg_event_queues_push_device(srg_event_queues* q, const srg_event_batch* batch_dev,
                                 const uint64_t* deliver_ns_dev, const uint32_t* order_dev, uint64_t num_order,
                                 const uint64_t* tag_dev, void* hip_stream, srg_queue_result* result, char* errbuf,
                                 size_t errlen);

/* Popped events grouped by host (increasing HostId), each host's in pop order;
 * out_host_offsets_dev[num_hosts + 1].  out_src_host_dev / out_src_event_id_dev may be NULL; with
 * out_capacity 0 every output may be NULL (a sizing call).  More than out_capacity events due:
 * SRG_ERR_ARG, num_moved = the count needed, nothing popped.                                     */
int srg_event_queues_pop_device(srg_event_queues* q, uint64_t until_ns, uint64_t out_capacity,
                                uint64_t* out_time_ns_dev, uint32_t* out_src_host_dev, uint64_t* out_src_event_id_dev,
                                uint64_t* out_tag_dev, uint64_t* out_host_offsets_dev, void* hip_stream,
                                srg_queue_result* result, char* errbuf, size_t errlen);

/* The controller's window step (controller.rs:88-112): start = min_next_event_ns; end =
 * min(start + runahead_ns (saturating at UINT64_MAX), end_time_ns).  Returns 1 and the window when
 * start < end, 0 when the simulation is over.  A usage error -- runahead_ns == 0 (the reference's
 * assert_ne!) or a null output -- returns -SRG_ERR_ARG: negative, because 1 already means "a
 * window".  No GPU work.                                                                        */
int srg_next_window(uint64_t min_next_event_ns, uint64_t runahead_ns, uint64_t end_time_ns,
                    uint64_t* window_start_ns, uint64_t* window_end_ns);

/* ---- the hosts' inbound path: CoDel router queue, token-bucket relay -------------------------
 * What every popped packet event begins with on its host (host.rs:853-858):
 *   router.route_incoming_packet(packet) -> CoDelQueue::push(packet, now)
 *                                              router/mod.rs:59-61, codel_queue.rs:305-319
 *   notify_router_has_packets()          -> relay_inet_in.notify(host)   host.rs:992-994, relay/mod.rs:111-136
 *   forward task -> forward_until_blocked: CoDelQueue::pop(now), TokenBucket::comforming_remove(total_size)
 *                                              relay/mod.rs:201-273, token_bucket.rs:68-157
 * kept per host in HBM across steps: the bucket (refill max(1, bw_down_bits / 8 / 1000) per 1 ms,
 * capacity refill + 1500, created full; bw_down_bits == UINT64_MAX is RateLimit::Unlimited), the
 * CoDel state (TARGET 10 ms, INTERVAL 100 ms, no length limit), the relay (Idle / Pending, one
 * cached packet) and the router queue's packets.  Per host: an arrival at t is enqueued with
 * enqueue_ts = t and, if the relay is Idle, schedules a forward task at t; a task at T runs after
 * every arrival with time <= T (Packet before Local, event.rs:103-110); before bootstrap_end_ns
 * the bucket is not touched.  A step processes every given arrival and every forward task with
 * time < until_ns; a task at exactly until_ns stays pending.
 *   Domain: sim_start_ns <= every time < 2^62, until_ns <= 2^62; outside it, offsets that are not
 *        monotone from 0 to num_arrivals, or an arrival time >= until_ns: SRG_ERR_ARG
 *   a packet larger than a limited host's bucket capacity: SRG_ERR_ARG (the balance is clamped to
 *        the capacity, so the reference's relay would reschedule itself every refill for ever;
 *        Shadow's packets are at most CONFIG_MTU and never get there)
 *   an arrival earlier than its host's previous arrival or its last executed task:
 *        SRG_ERR_TIME_BACKWARD
 * Outputs are grouped by host (increasing HostId), each host's packets in the order they left,
 * forwards (status 1, at the task's time) and CoDel drops (status 0, the time of the task that
 * dropped them) interleaved as they occurred.  With out_capacity 0 every output may be NULL; more
 * packets leaving than out_capacity: SRG_ERR_ARG, num_forwarded + num_dropped = the count needed,
 * nothing changed; (num_queued before the call) + num_arrivals always suffices.  Any call that
 * returns an error leaves the state exactly as it was.  The call returns after its stream work is
 * complete.  The caller folds min_next_wake_ns into the minimum it hands to srg_next_window: a
 * pending forward task is a local event of its host.
 *   Outside the call: the interface and sockets behind the relay (relay_inet_out, the upstream
 * bucket fed by the interface's socket scheduler, is srg_outbound_* below); the order between a
 * forward task and another local event of the same host at the same nanosecond (by event id in the
 * reference; it changes no output of this call).  With the CPU-delay model on, the caller passes the time at which each
 * packet event actually ran.                                                                     */
/* opaque; lives in the HBM of ctx's device; not thread-safe; destroy it before its ctx */
typedef struct srg_inbound srg_inbound;
/* bw_down_bits: host array [num_hosts] (srg_graph_node_bandwidth's value of the host's node);
 * reserve_packets: router-queue capacity allocated up front (growth reallocates geometrically) */
int srg_inbound_create(srg_ctx* ctx, uint32_t num_hosts, const uint64_t* bw_down_bits, uint64_t sim_start_ns,
                       uint64_t bootstrap_end_ns, uint64_t reserve_packets, srg_inbound** out, char* errbuf,
                       size_t errlen);
void srg_inbound_destroy(srg_inbound* q);

typedef struct srg_inbound_result {
    uint64_t num_forwarded, num_dropped; /* left the router in this step */
    uint64_t num_queued;                 /* still in router queues + cached packets, after the step */
    uint64_t min_next_wake_ns;           /* min pending forward-task time over hosts, UINT64_MAX if none */
    double ms_total;
} srg_inbound_result;

/* time_ns_dev, tag_dev, host_offsets_dev[num_hosts + 1]: exactly what srg_event_queues_pop_device
 * wrote; total_size_dev[num_arrivals]: each packet's total size (packet.total_size()).          */
int srg_inbound_step_device(srg_inbound* q, uint64_t until_ns, uint64_t num_arrivals, const uint64_t* time_ns_dev,
                            const uint32_t* total_size_dev, const uint64_t* tag_dev, const uint64_t* host_offsets_dev,
                            uint64_t out_capacity, uint8_t* out_status_dev, uint64_t* out_time_ns_dev,
                            uint64_t* out_tag_dev, uint64_t* out_host_offsets_dev, void* hip_stream,
                            srg_inbound_result* result, char* errbuf, size_t errlen);

/* (a struct tag, not a typedef: the read-back below has the same name) */
struct srg_inbound_host_state {
    uint64_t balance, last_refill_ns;       /* TokenBucket (balance 0 on an unlimited host) */
    uint64_t interval_end_ns, drop_next_ns; /* valid with has_interval_end / has_drop_next */
    uint64_t current_drop_count, previous_drop_count, bytes_stored;
    uint64_t queued;                        /* packets in the CoDel queue (the cached one is not) */
    uint64_t wake_ns, cached_tag;           /* valid with pending / has_cached */
    uint8_t mode;                           /* 0 Store, 1 Drop */
    uint8_t has_interval_end, has_drop_next, pending, has_cached, reserved[3];
};
/* one small read-back; SRG_ERR_ARG for host >= num_hosts */
int srg_inbound_host_state(srg_inbound* q, uint32_t host, struct srg_inbound_host_state* out);

/* ---- the hosts' outbound path: socket qdisc, upstream token bucket ---------------------------
 * What lies between a socket that has a packet and Worker::send_packet:
 *   notify_socket_has_packets(socket)     -> networkinterface_wantsSend, relay_inet_out.notify(host)
 *                                              host.rs:1003-1017, network_interface.c:344-370
 *   forward task -> forward_until_blocked: networkinterface_pop (the qdisc picks a socket, the socket
 *       gives its next packet), TokenBucket::comforming_remove(total_size), Router::push =
 *       Worker::send_packet          relay/mod.rs:166-273, network_interface.c:205-340, router/mod.rs:49-77
 * kept per host in HBM across steps: the sockets' packets (a socket is a slot; priority 0 is a
 * control packet and goes into the slot's control FIFO, any other priority into its data FIFO; the
 * slot's next packet is the control FIFO's head, else the data FIFO's: socket.c:198-199,437-442),
 * the qdisc structure, the bucket (refill max(1, bw_up_bits / 8 / 1000) per 1 ms, capacity refill +
 * 1500, created full; bw_up_bits == UINT64_MAX is RateLimit::Unlimited) and the relay (Idle /
 * Pending, one cached packet).
 *   SRG_QDISC_FIFO: the reference's binary heap of sockets, restated literally
 *       (utility/priority_queue.c:87-175, network_queuing_disciplines.c:82-160).  The heap stores no
 *       keys: a compare reads the two sockets' current next-packet priority, `a` is smaller than `b`
 *       unless prio(a) > prio(b) (equal keys compare as smaller both ways), an offer to a socket that
 *       is already in the heap re-sifts nothing (a control packet offered there leaves a stale
 *       position), pop moves the last entry to the root and sifts it down, preferring the right
 *       child only when it compares smaller than the left.  Equal non-zero priorities are accepted
 *       and ordered as this heap orders them.  It is not "the smallest queued priority".
 *   SRG_QDISC_ROUND_ROBIN: a plain queue of sockets; pop the head, pull its next packet, push it to
 *       the tail if it has more (network_interface.c:205-247).
 *   An offer (one packet entering slot `socket` at time_ns): a slot not in the structure is pushed
 *   into it; if the relay is Idle a forward task is scheduled at the offer's time.  The task at T
 *   loops: the cached packet, else the qdisc's selection step; none: Idle.  At T >= bootstrap_end_ns
 *   a packet without SRG_OFFER_LOCAL on a limited host removes total_size tokens; on failure the
 *   packet is cached and the task runs again at T + the conforming duration.  Otherwise the packet
 *   leaves at T: status 1, sent to the router -- out_time_ns is its srg_send_batch.send_time_ns --
 *   or status 2, a local packet (its destination is the host's own address: pushed back into the
 *   interface, no tokens, but it waits behind a cached packet like any other).
 *   Order of offers and tasks: in the reference a forward task is a local event, ordered by event id
 *   among its host's other local events of the same nanosecond; only the caller knows those ids, so
 *   an offer says it with one bit.  A host's offers are given in execution order with non-decreasing
 *   times.  Before offer i at time t is enqueued, every pending task with wake < t runs; a pending
 *   task with wake == t runs first if and only if the offer carries SRG_OFFER_BARRIER -- without the
 *   bit it runs after this offer and the following offers at t, up to the next barrier offer.  After
 *   the last offer every task with time < until_ns runs; a task at exactly until_ns stays pending.
 *   Without any barrier this is the inbound rule.  With the FIFO qdisc, unique increasing priorities
 *   and no control packets the bit changes no output; with control packets, or round robin, it does.
 *   Domain: sim_start_ns <= every time < 2^62, until_ns <= 2^62; outside it, offsets that are not
 *        monotone from 0 to num_offers, a time >= until_ns, a slot >= sockets_per_host[h], an unknown
 *        flag bit, a qdisc other than 0 or 1: SRG_ERR_ARG
 *   a packet without SRG_OFFER_LOCAL larger than a limited host's bucket capacity: SRG_ERR_ARG (a
 *        deviation shared with the inbound call: the balance is clamped to the capacity, so the
 *        reference's relay would reschedule itself every refill for ever)
 *   an offer earlier than its host's previous offer or its last executed task: SRG_ERR_TIME_BACKWARD
 * Outputs are grouped by host (increasing HostId), each host's packets in the order they left: the
 * order of the host's send_packet calls, so the order in which the caller draws `chance` and event
 * ids.  With out_capacity 0 every output may be NULL; more packets leaving than out_capacity:
 * SRG_ERR_ARG, num_sent + num_local = the count needed, nothing changed; (num_queued before the
 * call) + num_offers always suffices.  Any call that returns an error leaves the state exactly as it
 * was.  The call returns after its stream work is complete.  The caller folds min_next_wake_ns into
 * the minimum it hands to srg_next_window.
 *   Outside the call: the socket-buffer feedback to the process (the space a pulled packet frees),
 * relay_loopback, pcap and tracker side effects.                                                 */
#define SRG_QDISC_FIFO 0
#define SRG_QDISC_ROUND_ROBIN 1
#define SRG_OFFER_LOCAL 1u   /* dst is the host's own address: no tokens, status 2 */
#define SRG_OFFER_BARRIER 2u /* a forward task due at this offer's time runs before it */
/* opaque; lives in the HBM of ctx's device; not thread-safe; destroy it before its ctx */
typedef struct srg_outbound srg_outbound;
/* bw_up_bits, sockets_per_host: host arrays [num_hosts] (srg_graph_node_bandwidths' host_bandwidth_up
 * of the host's node; the number of socket slots of the host, below 2^31); reserve_packets: socket
 * capacity allocated up front (growth reallocates geometrically) */
int srg_outbound_create(srg_ctx* ctx, uint32_t num_hosts, const uint64_t* bw_up_bits, const uint32_t* sockets_per_host,
                        int qdisc, uint64_t sim_start_ns, uint64_t bootstrap_end_ns, uint64_t reserve_packets,
                        srg_outbound** out, char* errbuf, size_t errlen);
void srg_outbound_destroy(srg_outbound* q);

typedef struct srg_outbound_result {
    uint64_t num_sent, num_local; /* left in this step: to the router / back into the interface */
    uint64_t num_queued;          /* still in sockets + cached packets, after the step */
    uint64_t min_next_wake_ns;    /* min pending forward-task time over hosts, UINT64_MAX if none */
    double ms_total;
} srg_outbound_result;

/* The offers, grouped by host (host_offsets_dev[num_hosts + 1]), each host's in execution order:
 * time_ns_dev, socket_dev (slot < sockets_per_host[h]), priority_dev (0: control), total_size_dev,
 * flags_dev (SRG_OFFER_*; NULL = all 0), tag_dev (the caller's handle, returned in out_tag_dev).
 * out_status_dev: 1 sent to the router, 2 local.                                                */
int srg_outbound_step_device(srg_outbound* q, uint64_t until_ns, uint64_t num_offers, const uint64_t* time_ns_dev,
                             const uint32_t* socket_dev, const uint64_t* priority_dev, const uint32_t* total_size_dev,
                             const uint8_t* flags_dev, const uint64_t* tag_dev, const uint64_t* host_offsets_dev,
                             uint64_t out_capacity, uint8_t* out_status_dev, uint64_t* out_time_ns_dev,
                             uint64_t* out_tag_dev, uint64_t* out_host_offsets_dev, void* hip_stream,
                             srg_outbound_result* result, char* errbuf, size_t errlen);

/* (a struct tag, not a typedef: the read-back below has the same name) */
struct srg_outbound_host_state {
    uint64_t balance, last_refill_ns; /* TokenBucket (balance 0 on an unlimited host) */
    uint64_t wake_ns, cached_tag;     /* valid with pending / has_cached */
    uint64_t queued;                  /* packets in the host's sockets (the cached one is not) */
    uint32_t qdisc_len;               /* sockets in the heap / the round-robin queue */
    uint8_t pending, has_cached, reserved[2];
};
/* one small read-back; SRG_ERR_ARG for host >= num_hosts */
int srg_outbound_host_state(srg_outbound* q, uint32_t host, struct srg_outbound_host_state* out);
/* the heap array (or the round-robin queue from its head) in array order: *n slots, the first
 * min(*n, capacity) of them in slots[]; SRG_ERR_ARG for host >= num_hosts */
int srg_outbound_host_order(srg_outbound* q, uint32_t host, uint32_t* slots, uint32_t capacity, uint32_t* n);

/* ---- a round on the device: packet table, per-host RNG and event ids --------------------------
 * The five calls above, joined: a round is srg_round_receive_device, the hosts run, then
 * srg_round_send_device, and srg_next_window(result.next_start_ns, ...).  What joined them on the
 * host before lives in HBM: each host's random generator, its event-id counter, the hosts' nodes
 * and a packet table indexed by tag, so nothing of a round's packets crosses to the host.
 *   Host::random          Xoshiro256PlusPlus::seed_from_u64(node_seed)     host.rs:122,233
 *   chance                src_host.random_mut().gen::<f64>()               worker.rs:377
 *                         = (next_u64() >> 11) * 2^-53, one generator step (rand 0.8.5)
 *   is_completed          current_time >= sim_end_time: return, no draw    worker.rs:336-343
 *   unknown destination   PDS_INET_DROPPED, return, no draw                worker.rs:352-368
 *   the drop decision     after the draw; bootstrap and payload 0 draw too worker.rs:382-390
 *   the event id          Event::new_packet inside push_packet_to_host: behind the drop return, so a
 *                         packet dropped by loss takes none       worker.rs:422,644-654, event.rs:18-31
 *                         the counter starts at 0 and is the host's own    host.rs:258,690-694
 * The ids differ from the reference's by the host's local events (they share the counter); the
 * pop order does not: ids are only compared between events of one source host, and both
 * assignments strictly increase in that host's send order (round_rule.h derives it).
 *   Send half: the offers are checked and completed from the packet table (total_size gathered;
 * SRG_OFFER_LOCAL derived as dst_host == the offering host, the caller's flag byte may carry only
 * SRG_OFFER_BARRIER), the outbound step runs, every packet that left for the router is classified
 * and, if it draws, drawn for in its host's leaving order, the drawing packets go through the send
 * batch (round_end_ns = until_ns) and the sent ones are pushed into the queues.
 *   Receive half: pop(until_ns), each popped packet's total_size from the table, the inbound step.
 *   SRG_ERR_ARG: a tag >= num_packets; a dst_host that is neither < num_hosts nor SRG_NO_HOST; a flag
 * bit other than the barrier; a non-local packet above its DESTINATION's downstream bucket
 * (refill + 1500; this is what makes the inbound step's size error impossible later); no packet
 * table; whatever the composed calls refuse, with their codes (SRG_ERR_TIME_BACKWARD,
 * SRG_ERR_EVENT_ORDER, SRG_ERR_LATENCY_RANGE).
 *   Any call that returns an error leaves everything exactly as it was: the three parts, the
 * generators and the counters.  packet_counts_dev is the one exception, as in
 * srg_send_packets_device.  Both calls return after their stream work is complete.
 *   Outputs are borrowed device pointers in the result, owned by the object: the send half's are
 * valid until the next send, the receive half's until the next receive.  They are sized by the
 * bounds the parts give (queued before + arrivals always suffices), so there is no capacity error.
 *   Outside the calls: a host's other draws from the same generator (getrandom, port selection)
 * and its local events' ids.  Between two calls the caller folds them in with srg_round_host_rng /
 * srg_round_set_host_rng: read the state, step it, write it back.  Draws of other consumers INSIDE
 * a step -- between two send_packet calls of one window -- are outside the call: the step draws
 * its packets' chances back to back.                                                            */
#define SRG_NO_HOST 0xFFFFFFFFu  /* dst_host of a packet whose destination address no host owns */
#define SRG_ROUND_DROPPED 0      /* drew, dropped by loss */
#define SRG_ROUND_SENT 1         /* drew, took an event id, entered its destination's queue */
#define SRG_ROUND_LOCAL 2        /* left for the host's own address: never reaches send_packet */
#define SRG_ROUND_AFTER_END 3    /* left at >= sim_end_ns: no draw, no id */
#define SRG_ROUND_NO_HOST 4      /* dst_host == SRG_NO_HOST: no draw, no id */
/* opaque; lives in the HBM of ctx's device; not thread-safe; destroy it before its ctx */
typedef struct srg_round srg_round;
/* host arrays [num_hosts]: host_node (the host's position in `table`, < table->n), bw_up_bits,
 * bw_down_bits, sockets_per_host, node_seed (HostParameters::node_seed).  `table`: the struct is
 * copied, its device arrays are borrowed for the object's life (the rules of
 * srg_send_packets_device; packet_loss NULL: nothing is dropped, every packet still draws).
 * reserve_packets goes to the three parts.                                                      */
int srg_round_create(srg_ctx* ctx, uint32_t num_hosts, const uint32_t* host_node, const srg_path_table_dev* table,
                     const uint64_t* bw_up_bits, const uint64_t* bw_down_bits, const uint32_t* sockets_per_host,
                     int qdisc, const uint64_t* node_seed, uint64_t sim_start_ns, uint64_t bootstrap_end_ns,
                     uint64_t sim_end_ns, uint64_t reserve_packets, srg_round** out, char* errbuf, size_t errlen);
void srg_round_destroy(srg_round* r);
/* The caller's packet pool, indexed by tag, borrowed (device arrays [num_packets]); may be called
 * again when the pool grows or moves.  Entries of packets still inside the round object (in a
 * socket, a queue or a router) must not change.                                                 */
int srg_round_set_packets(srg_round* r, uint64_t num_packets, const uint32_t* dst_host_dev,
                          const uint32_t* total_size_dev, const uint32_t* payload_size_dev);

typedef struct srg_round_receive_result {
    uint64_t num_popped;                     /* events popped: the inbound step's arrivals */
    const uint64_t* popped_time_ns_dev;      /* [num_popped] grouped by host, pop order */
    const uint64_t* popped_tag_dev;          /* [num_popped] */
    const uint64_t* popped_host_offsets_dev; /* [num_hosts + 1] */
    uint64_t num_leaving;                    /* = num_forwarded + num_dropped: the inbound step's outputs */
    const uint8_t* status_dev;               /* [num_leaving] 1 forwarded, 0 dropped by CoDel */
    const uint64_t* time_ns_dev;             /* [num_leaving] */
    const uint64_t* tag_dev;                 /* [num_leaving] */
    const uint64_t* host_offsets_dev;        /* [num_hosts + 1] */
    uint64_t num_forwarded, num_dropped;
    uint64_t num_queued_inbound, num_queued_events; /* after the call */
    uint64_t min_next_event_ns, min_inbound_wake_ns, min_outbound_wake_ns;
    uint64_t next_start_ns;                  /* their minimum: srg_next_window's first argument */
    double ms_total;
} srg_round_receive_result;

int srg_round_receive_device(srg_round* r, uint64_t until_ns, void* hip_stream, srg_round_receive_result* result,
                             char* errbuf, size_t errlen);

typedef struct srg_round_send_result {
    uint64_t num_leaving;             /* packets that left the outbound step */
    const uint8_t* status_dev;        /* [num_leaving] SRG_ROUND_*, grouped by host, leaving order */
    const uint64_t* time_ns_dev;      /* [num_leaving] leave time */
    const uint64_t* tag_dev;          /* [num_leaving] */
    const uint64_t* host_offsets_dev; /* [num_hosts + 1] */
    uint64_t num_sent, num_dropped, num_local, num_after_end, num_no_host; /* sum = num_leaving */
    uint64_t num_queued_outbound, num_queued_events; /* after the call */
    uint64_t min_used_latency_ns;     /* over the sent packets, UINT64_MAX if none */
    uint64_t min_next_event_ns, min_inbound_wake_ns, min_outbound_wake_ns;
    uint64_t next_start_ns;           /* their minimum: srg_next_window's first argument */
    double ms_total;
} srg_round_send_result;

/* The offers as srg_outbound_step_device takes them, without total_size (gathered by tag) and with
 * flags_dev carrying SRG_OFFER_BARRIER only (NULL = all 0).                                      */
int srg_round_send_device(srg_round* r, uint64_t until_ns, uint64_t num_offers, const uint64_t* time_ns_dev,
                          const uint32_t* socket_dev, const uint64_t* priority_dev, const uint8_t* flags_dev,
                          const uint64_t* tag_dev, const uint64_t* host_offsets_dev,
                          uint64_t* packet_counts_dev /* may be NULL */, void* hip_stream,
                          srg_round_send_result* result, char* errbuf, size_t errlen);

/* One host's generator words and next event id: small read-back / write.  SRG_ERR_ARG for
 * host >= num_hosts and for the all-zero state.                                                 */
int srg_round_host_rng(srg_round* r, uint32_t host, uint64_t words[4], uint64_t* next_event_id);
int srg_round_set_host_rng(srg_round* r, uint32_t host, const uint64_t words[4], uint64_t next_event_id);
/* Borrowed handles of the parts, for the *_host_state / _host_order read-backs.  Stepping, pushing
 * or popping a part through its handle, or destroying it, is a usage error: the round object owns
 * the order of their calls.                                                                     */
srg_event_queues* srg_round_queues(srg_round* r);
srg_inbound* srg_round_inbound(srg_round* r);
srg_outbound* srg_round_outbound(srg_round* r);

/* ---- interface receive: socket lookup, UDP receive buffers, tracker input counters ------------
 * What the inbound relay does with a packet it forwards (relay/mod.rs:261-271): dst.push(packet) ->
 *   networkinterface_push               network_interface.c:140-202: the socket associated with
 *                                       (protocol, dst port, src ip, src port), else the one
 *                                       associated with (protocol, dst port, 0, 0); none:
 *                                       PDS_RCV_INTERFACE_DROPPED
 *   inetsocket_pushInPacket             UdpSocket::push_in_packet, udp.rs:108-168: the connect() peer
 *                                       filter on the whole SocketAddrV4 (:116-135), then the receive
 *                                       buffer (MessageBuffer, udp.rs:1081-1157) with its soft limit
 *   tracker_addInputBytes               if and only if a socket was found, network_interface.c:192-197,
 *                                       tracker.c:188-252
 * kept in HBM across steps: per socket slot (host, slot < sockets_per_host[h]) its kind, its peer,
 * soft_limit_bytes, len_bytes and its buffered messages (tag, recv_time, payload); per host the five
 * remote-in counters; the association table.  The interface's own address in the reference's key is
 * constant per host: the host id stands for it.
 *   A delivery (one packet, by tag, at time t on host h), in this order:
 *     lookup   (h, protocol, dst_port, src_ip, src_port), else (h, protocol, dst_port, 0, 0)
 *     none     SRG_RCV_NO_SOCKET, slot UINT32_MAX, not counted
 *     found    counted whatever happens next: payload 0 -> packets_control += 1, bytes_control_header
 *              += total - payload; else packets_data += 1, bytes_data_header += total - payload,
 *              bytes_data_payload += payload (no retransmit classes, no per-socket stats; this is
 *              the internet interface, so these are the remote-in counters)
 *     EXTERNAL slot (the caller owns the socket's buffer, TCP for one): SRG_RCV_EXTERNAL, untouched
 *     UDP slot has_peer and (src_ip, src_port) != peer: SRG_RCV_PEER_MISMATCH; len_bytes >=
 *              soft_limit_bytes: SRG_RCV_FULL; else the message (tag, recv_time = t, payload) goes to
 *              the back, len_bytes += payload: SRG_RCV_BUFFERED.  The limit is soft: one message may
 *              carry len_bytes past it; payload 0 messages never fill a buffer; limit 0 refuses all.
 *   A read (one recvmsg on (h, slot) at time t, udp.rs:497-546): empty -> status 0 (EWOULDBLOCK);
 *   else status 1 and the front message's tag, recv_time and payload; it is popped (len_bytes -=
 *   payload) unless the read carries SRG_READ_PEEK.  Truncation to the user's buffer is the caller's.
 *   Order on a host: its deliveries in the order given, its reads in execution order, both with
 *   non-decreasing times.  A read at t runs after every delivery with time < t, and before the
 *   deliveries at t if and only if it carries SRG_READ_FIRST (both are local events of one
 *   nanosecond in the reference, ordered by event id; the same one-bit answer as SRG_OFFER_BARRIER).
 *   The buffers have no clock: nothing is checked across calls, call order is execution order.
 *   SRG_ERR_ARG: offsets that are not monotone from 0 to the count; a tag >= num_packets; no packet
 *        table; an unknown read flag; a read on a slot >= sockets_per_host[h] or on an EXTERNAL
 *        slot; a read with SRG_READ_FIRST behind a read without it at the same time on one host
 *        (the two contradict: the first ran after the deliveries at t, the second before them);
 *        rows + reads >= 2^31
 *   SRG_ERR_TIME_BACKWARD: a delivery (a read) earlier than its host's previous delivery (read)
 *   Any call that returns an error leaves the state exactly as it was: buffers, counters,
 * associations, configuration.  (The output arrays of a failed step are unspecified.)  The step
 * returns after its stream work is complete.
 *   Outside the calls: TCP's own receive path, the loopback interface, pcap, per-socket tracker
 * stats, the readable / writable callbacks (derive them from the per-delivery status).          */
#define SRG_SOCK_UDP 0
#define SRG_SOCK_EXTERNAL 1
#define SRG_RCV_SKIPPED 0       /* the row's status differs from deliver_status: not a delivery */
#define SRG_RCV_NO_SOCKET 1     /* PDS_RCV_INTERFACE_DROPPED */
#define SRG_RCV_EXTERNAL 2      /* found an EXTERNAL slot: the caller's socket takes it */
#define SRG_RCV_PEER_MISMATCH 3 /* PDS_RCV_SOCKET_DROPPED by the peer filter */
#define SRG_RCV_FULL 4          /* PDS_RCV_SOCKET_DROPPED by has_space */
#define SRG_RCV_BUFFERED 5      /* PDS_RCV_SOCKET_BUFFERED */
#define SRG_READ_PEEK 1u        /* MSG_PEEK: the message stays */
#define SRG_READ_FIRST 2u       /* the read runs before the deliveries of its own nanosecond */
#define SRG_SOCK_DEFAULT_RECV_BYTES 174760u /* CONFIG_RECV_BUFFER_SIZE, a new slot's soft limit */
/* opaque; lives in the HBM of ctx's device; not thread-safe; destroy it before its ctx */
typedef struct srg_sockets_in srg_sockets_in;
/* sockets_per_host: host array [num_hosts], its sum below 2^31.  Every slot starts as a UDP slot
 * without a peer, limit SRG_SOCK_DEFAULT_RECV_BYTES, empty.  reserve_messages: message storage
 * allocated up front (growth reallocates geometrically).                                        */
int srg_sockets_in_create(srg_ctx* ctx, uint32_t num_hosts, const uint32_t* sockets_per_host, uint64_t reserve_messages,
                          srg_sockets_in** out, char* errbuf, size_t errlen);
void srg_sockets_in_destroy(srg_sockets_in* q);
/* The caller's packet pool, indexed by tag, borrowed (device arrays [num_packets]); may be called
 * again when the pool grows or moves.  Entries of packets named by a step's rows must be valid
 * during the step; a buffered message keeps its own tag, time and payload.                     */
int srg_sockets_in_set_packets(srg_sockets_in* q, uint64_t num_packets, const uint8_t* protocol_dev,
                               const uint32_t* src_ip_dev, const uint16_t* src_port_dev, const uint16_t* dst_port_dev,
                               const uint32_t* total_size_dev, const uint32_t* payload_size_dev);
/* Batch calls between steps, host arrays [n].  configure sets a slot's kind, peer (udp.rs:116-135)
 * and limit; the limit of a non-empty buffer may change (set_soft_limit_bytes, udp.rs:1154); a slot
 * named twice keeps its last entry; the buffer of a slot that becomes EXTERNAL stays as it is.
 * associate: a key that exists already, also earlier in the same batch, is SRG_ERR_ARG
 * (utility_debugAssert, network_interface.c:85) and nothing of the batch is added.  disassociate:
 * a missing key is a no-op (network_interface.c:99-117).  A host >= num_hosts, a slot >=
 * sockets_per_host[host], a kind or has_peer above 1: SRG_ERR_ARG, nothing changed.  The device
 * table is rebuilt by the first step after a change.                                            */
int srg_sockets_in_configure(srg_sockets_in* q, uint64_t n, const uint32_t* host, const uint32_t* slot, const uint8_t* kind,
                             const uint8_t* has_peer, const uint32_t* peer_ip, const uint16_t* peer_port,
                             const uint64_t* soft_limit_bytes, char* errbuf, size_t errlen);
int srg_sockets_in_associate(srg_sockets_in* q, uint64_t n, const uint32_t* host, const uint8_t* protocol,
                             const uint16_t* local_port, const uint32_t* peer_ip, const uint16_t* peer_port,
                             const uint32_t* slot, char* errbuf, size_t errlen);
int srg_sockets_in_disassociate(srg_sockets_in* q, uint64_t n, const uint32_t* host, const uint8_t* protocol,
                                const uint16_t* local_port, const uint32_t* peer_ip, const uint16_t* peer_port,
                                char* errbuf, size_t errlen);

typedef struct srg_sockets_in_result {
    uint64_t num_skipped, num_no_socket, num_external, num_peer_mismatch, num_full, num_buffered; /* rows per status */
    uint64_t num_read, num_would_block; /* reads with status 1 / 0 */
    uint64_t num_buffered_messages;     /* in all buffers, after the step */
    double ms_total;
} srg_sockets_in_result;

/* Rows: status_dev, time_ns_dev, tag_dev, host_offsets_dev[num_hosts + 1] exactly as
 * srg_inbound_step_device or srg_round_receive_result give them (deliver_status 1: the forwarded
 * packets) or as srg_round_send_result gives them (deliver_status SRG_ROUND_LOCAL: the packets the
 * relay pushes back into the interface, relay/mod.rs:263-266); a row whose status differs is
 * skipped; status_dev NULL: every row is a delivery.  Reads: read_time_ns_dev, read_slot_dev,
 * read_flags_dev (SRG_READ_*; NULL = all 0), read_host_offsets_dev[num_hosts + 1]; with a count of 0
 * the arrays, offsets included, may be NULL.
 * Outputs: out_status_dev[num_rows] SRG_RCV_*, out_slot_dev[num_rows] (UINT32_MAX: no socket or
 * skipped); out_read_status_dev[num_reads] 1 / 0, and the message's tag, recv_time and payload
 * (0 with status 0).                                                                            */
int srg_sockets_in_step_device(srg_sockets_in* q, uint64_t num_rows, const uint8_t* status_dev,
                               const uint64_t* time_ns_dev, const uint64_t* tag_dev, const uint64_t* host_offsets_dev,
                               uint8_t deliver_status, uint64_t num_reads, const uint64_t* read_time_ns_dev,
                               const uint32_t* read_slot_dev, const uint8_t* read_flags_dev,
                               const uint64_t* read_host_offsets_dev, uint8_t* out_status_dev, uint32_t* out_slot_dev,
                               uint8_t* out_read_status_dev, uint64_t* out_read_tag_dev, uint64_t* out_read_time_ns_dev,
                               uint32_t* out_read_payload_dev, void* hip_stream, srg_sockets_in_result* result,
                               char* errbuf, size_t errlen);

/* (struct tags, not typedefs: the read-backs below have the same names) */
struct srg_sockets_in_socket_state {
    uint64_t len_bytes, num_messages, soft_limit_bytes;
    uint32_t peer_ip;
    uint16_t peer_port;
    uint8_t kind, has_peer;
};
struct srg_sockets_in_host_counters {
    uint64_t packets_control, packets_data, bytes_control_header, bytes_data_header, bytes_data_payload;
};
/* one small read-back each; SRG_ERR_ARG for a host or slot out of range.  reset != 0 zeroes the
 * host's counters after reading them, as the heartbeat does (tracker.c:608).                    */
int srg_sockets_in_socket_state(srg_sockets_in* q, uint32_t host, uint32_t slot, struct srg_sockets_in_socket_state* out);
int srg_sockets_in_host_counters(srg_sockets_in* q, uint32_t host, struct srg_sockets_in_host_counters* out, int reset);

/* ---- the routes a table's paths take; per-edge packet loads --------------------------------
 * The reference keeps no routes: petgraph's dijkstra returns scores only (mod.rs:190-208).  They
 * can be read back from a finished shortest-path table alone, because a Dijkstra label is
 * label(u) + edge (PathProperties::add, mod.rs:321-331: the latency adds, the loss is the f32 left
 * fold 1 - (1 - L)(1 - p)): for every s != t the table holds a vertex u and an in-edge e = (u, t)
 * with D[s][u] + lat(e) == D[s][t] and bits(fold(L[s][u], loss(e))) == bits(L[s][t]), the source's
 * own label being (0, +0.0f), not the diagonal (which holds the raw self-loop weight).  Walking
 * that relation back from t gives a route; no buffer of the build is used, so a table of either
 * build, in either form of srg_path_table_dev, from one rank or many, is traced the same way.
 *   Tie rule (makes the route unique): in-edges of a vertex are the edges (u, cur), u != cur; on an
 *   undirected graph an edge stored as (cur, u) counts too; self-loops are never candidates; among
 *   the in-edges that satisfy both equalities the one with the SMALLEST EDGE INDEX (position in
 *   srg_edge_list) is the route's edge.
 *   The route is *a* minimal path reproducing the table's (latency, loss) bits, made unique by the
 *   tie rule; the reference's own choice among bit-equal predecessors is unobservable.
 *   Diagonal: the route s -> s is one hop, the self-loop edge of s (mod.rs:210-217; the smallest
 *   index if the list holds several); none: SRG_ERR_NO_EDGE with the reference's text.
 *   Table shape: the table must cover every vertex in NodeIndex order (table->n == num_vertices,
 *   position = vertex) and table->packet_loss is required; anything else is SRG_ERR_ARG.
 *   Rectangular or subset tables are out of scope.
 *   A query index >= n is SRG_ERR_ARG; so is an edge of latency 0 between two vertices in
 *   graph_dev (the walk ends because latencies are >= 1; a hop cap of num_vertices backs that up).
 *   A get_direct_paths table is not a fold from (0, 0) and is refused with SRG_ERR_ROUTE: its
 *   routes are the single edges.
 *   The in-edge lists are rebuilt from graph_dev on every call (nothing is cached between calls:
 *   the edge arrays may be rewritten in place); the workspace is the context's.
 *   Both calls return after their stream work is complete, and leave the hop arrays, the offsets
 *   and edge_packets_dev untouched on any error: every pair is walked first, then committed.   */
#define SRG_ERR_ROUTE 13   /* a pair whose table entry no in-edge explains: the table is not a
                              shortest-path table of this graph (wrong graph, a direct-path table,
                              a damaged entry) */
typedef struct srg_route_result {
    uint64_t num_pairs;    /* pairs walked (loads: the nonzero count entries) */
    uint64_t total_hops;   /* sum of route lengths (trace: also the capacity needed) */
    uint64_t bad_pair;     /* SRG_ERR_ROUTE: index of the first unexplained query (loads: s*n+t);
                              else UINT64_MAX */
    uint32_t max_hops, reserved;
    double ms_total;
} srg_route_result;

/* Device pointers throughout.  Query i is the path src_dev[i] -> dst_dev[i] (NodeIndex values).
 * Its route is out_hop_edge_dev[out_hop_offsets_dev[i] .. out_hop_offsets_dev[i + 1]), edge indices
 * in order from s to t; out_hop_vertex_dev (same slots) is the vertex each hop arrives at, so the
 * last one is t.  Sizing as srg_event_queues_pop_device: with hop_capacity 0 every output may be
 * NULL; more hops needed than hop_capacity: SRG_ERR_ARG, total_hops = the need, nothing written.
 * SRG_ERR_ROUTE names the pair (the source's and the target's NodeIndex) in errbuf.
 * num_pairs < 2^31 - 1.                                                                        */
int srg_trace_routes_device(srg_ctx* ctx, const srg_edge_list* graph_dev, const srg_path_table_dev* table,
                            const uint32_t* src_dev, const uint32_t* dst_dev, uint64_t num_pairs,
                            uint64_t hop_capacity, uint64_t* out_hop_offsets_dev /* [num_pairs+1] */,
                            uint32_t* out_hop_edge_dev /* [hop_capacity] edge indices, s -> t */,
                            uint32_t* out_hop_vertex_dev /* may be NULL: the vertex each hop arrives at */,
                            void* hip_stream, srg_route_result* result, char* errbuf, size_t errlen);

/* Per-edge packet loads: every nonzero entry [s, t] of a packet-count table (what
 * srg_send_packets_device accumulates) is added to every edge of the route s -> t; a diagonal
 * count goes to the self-loop edge.  Saturating at UINT64_MAX.  n * n < 2^31 - 1.              */
int srg_link_loads_device(srg_ctx* ctx, const srg_edge_list* graph_dev, const srg_path_table_dev* table,
                          const uint64_t* packet_counts_dev /* [n*n] by position */,
                          uint64_t* edge_packets_dev /* [num_edges], NOT cleared: accumulated, saturating */,
                          void* hip_stream, srg_route_result* result, char* errbuf, size_t errlen);

/* ---- route trees: predecessor, hop and first-hop tables; link loads by tree -------------------
 * For one source s the routes above to all targets form a tree: the tie rule makes every route
 * unique, and the route to t through u ends with the route to u.  The two calls below work on whole
 * source rows of that tree where the two above walk one pair at a time.
 *   Essential in-edges.  A route edge (u, t) is itself a shortest path u -> t, so only edges with
 *   lat(e) == D[u][t] can match; on a shortest-path table that filter removes no candidate of any
 *   row and leaves the tie rule's minimum unchanged.  The filter reads the entries (u, t) of EVERY
 *   row an edge starts from, requested or not: it trusts them.  An edge with lat(e) < D[u][t]
 *   proves that the table is not this graph's.
 *   Batches.  Rows are processed in batches (SRG_OPT_ROUTE_TREE_ROWS); by default a batch is as
 *   many rows as a workspace budget of 4 GiB allows (per table entry of a batch: 16 B of doubling
 *   scratch when n > 4096; srg_route_trees_device 4 B more when out_pred_vertex_dev is NULL;
 *   srg_link_loads_trees_device 12 B more).  The workspace is the context's.
 *   Which call for loads.  Measured on an MI355X on the 10 000-vertex bench table (DESIGN.md
 *   §11.1): the tree call takes 257 ms whether 10^6, 10^7 or all 10^8 entries are nonzero (its
 *   cost is per row holding a nonzero, 26 us each there), the pairwise call 495 ms for 10^6 and
 *   4 463 ms for 10^7 nonzero pairs (0.45 - 0.49 us per pair).  Prefer this call from some tens of
 *   nonzero pairs per nonzero row (about 55 on that table), srg_link_loads_device for a sparser
 *   table or a few rows, and this call whenever n * n >= 2^31 - 1.                              */
#define SRG_ROUTE_NONE 0xFFFFFFFFu   /* no edge / no vertex (the source's own column) */

/* The route tree of each listed source, from the table and the graph alone (same rule, same tie
 * rule, same table-shape requirements as srg_trace_routes_device).  Row i belongs to source
 * sources_dev[i] (NULL: source i; then num_sources <= n); duplicates allowed.  For column t != s:
 *   pred_edge   = the route's last edge (into t), pred_vertex = the vertex it comes from,
 *   hops        = the route's length, first_edge = the route's first edge (out of s).
 * Column t == s: SRG_ROUTE_NONE, hops 0 (the self-loop route stays with srg_trace_routes_device).
 * result: num_pairs = num_sources * (n - 1), total_hops, max_hops over all of them; bad_pair =
 * i * n + t (i the row index) of the smallest entry no in-edge explains (SRG_ERR_ROUTE), or
 * u * n + t of an edge (u, t) whose latency is below the table's entry (u, t) (SRG_ERR_ROUTE too),
 * else UINT64_MAX.  SRG_ERR_ARG: what the table-shape rules refuse, a source >= n, num_sources > 0
 * with out_pred_edge_dev NULL, a zero-latency edge between two vertices, an endpoint >= n.
 * num_sources == 0 is SRG_OK and touches nothing.  The four arrays are pure outputs: on any error
 * their contents are unspecified.  Returns after its stream work is complete.                  */
int srg_route_trees_device(srg_ctx* ctx, const srg_edge_list* graph_dev, const srg_path_table_dev* table,
                           const uint32_t* sources_dev, uint32_t num_sources,
                           uint32_t* out_pred_edge_dev   /* [num_sources * n] */,
                           uint32_t* out_pred_vertex_dev /* may be NULL */,
                           uint32_t* out_hops_dev        /* may be NULL */,
                           uint32_t* out_first_edge_dev  /* may be NULL */,
                           void* hip_stream, srg_route_result* result, char* errbuf, size_t errlen);

/* srg_link_loads_device's contract and results, computed per source row through the route tree;
 * no limit on n * n.  Every row holding a nonzero count gets its tree; the counts are pushed from
 * the deepest level up (the load of the edge into t is the count of the subtree under t, the sums
 * saturating like the loads).  Only vertices on the route of a nonzero pair have to be explained.
 * Every batch is validated before anything is committed: any error leaves edge_packets_dev
 * untouched.  Should the essential lists not explain a nonzero pair, or an edge lie below its
 * entry, the call repeats itself with the full in-edge lists, so it fails exactly where
 * srg_link_loads_device does.  A tree of depth d costs d sweeps over its row: a chain is slow.  */
int srg_link_loads_trees_device(srg_ctx* ctx, const srg_edge_list* graph_dev, const srg_path_table_dev* table,
                                const uint64_t* packet_counts_dev, uint64_t* edge_packets_dev,
                                void* hip_stream, srg_route_result* result, char* errbuf, size_t errlen);

/* Library build/version string. */
const char* srg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SHADOW_ROUTING_H */
