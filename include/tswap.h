/*
 * tswap.h — C ABI of the MI355X-native TSWAP planning core (libtswap_hip.so).
 *
 * Drop-in boundary for the reference's src/algorithm path
 * (RenKoya1/p2p_distributed_tswap @ 2025-11-21). Plain pointers and sizes,
 * no torch types. Every call is synchronous for the caller (like the
 * reference); device work runs on the context's own HIP stream.
 *
 * Coordinates: Point = (x, y) with x = column, y = row, grid[y][x]
 * (src/map/map.rs:4, tswap.rs:53). Cell id = y*w + x. A cell is blocked iff
 * its byte is '@' (tswap.rs:53); every other byte is passable.
 *
 * Errors: 0 on success, negative errno-style code otherwise; the reference
 * panics where these return TSW_EINVAL (tswap.rs:94,112,136).
 * tsw_last_error(ctx) gives the message of the last failure. A failed call
 * leaves the context consistent: no goal stays registered against a partial
 * table and no next hop stays queued for a K3 pass that did not run.
 * One context is single-threaded; separate contexts may live on separate
 * threads or devices.
 *
 * Hard limits where the reference (usize arithmetic, unbounded Vec/HashMap)
 * would keep going — each returns an error code, never a wrong answer:
 *   - grid: at most 2048 cells per side and 2^20 cells      (tsw_create -> NULL)
 *   - BFS distances are u16: a goal whose farthest reachable cell is more than
 *     65534 steps away (only possible on grids of more than 65535 free cells,
 *     e.g. a serpentine maze) has no distance table. Planning entry points
 *     (tsw_plan_mapd, tsw_step, tsw_decide, tsw_next_hop_tables) keep such a goal
 *     WITHOUT a table and resolve every next hop toward it with the exact A*
 *     (K3, 20-bit g): same results, slower. The table-returning entry points
 *     (tsw_dist_tables*, tsw_next_hop_tables_device) return TSW_EOVERFLOW for it.
 *   - exact A*: the LDS-heap kernels hand queries with g >= 2^15, f >= 2^17 or
 *     a heap past their LDS capacity to the global-heap kernel (20-bit g, enough
 *     for any path on a 2^20-cell grid); its heap holds min(4*cells+8, 65536)
 *     entries, past that TSW_EOVERFLOW
 *   - tsw_decide, tsw_decide_fleet: at most 1024 entries in one agent's nearby list (TSW_EOVERFLOW
 *     when a longer list reaches Rule 4; get_nearby, decentralized/agent.rs:108-153, has no bound)
 *   - tsw_nearby, tsw_decide_fleet: the lists of one call hold at most 2^32 - 1 entries (TSW_EOVERFLOW)
 *   - goal tables: table_budget_bytes (2 B per cell per goal). Tables not used by
 *     the current call are evicted least-recently-used first; TSW_ENOMEM only
 *     when the goals of ONE call do not fit.
 *
 * Device-memory arguments (*_device entry points) may be produced on any stream
 * of the caller: the library synchronises the device before reading or writing
 * them, and the call has completed its device work when it returns.
 */
#ifndef TSWAP_H
#define TSWAP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSW_OK 0
#define TSW_EINVAL (-22)
#define TSW_ENOMEM (-12)
#define TSW_EHIP (-5)
#define TSW_EOVERFLOW (-75)
#define TSW_ENODEV (-19)

/* Revision of this ABI: bumped whenever a struct or a signature changes, so a caller
 * built against an older header can refuse to run. 3: tsw_opts grew to 24 bytes (watchdog_ms),
 * tsw_next_hop_tables_device gained dev_dist; 4: tsw_abi_version, lazy task-cell checks,
 * tsw_plan_mapd_resolved / tsw_next_hop_codes; 5: tsw_build_id, entry points refuse re-entry from a
 * tsw_plan_mapd_resolved resolver (TSW_EINVAL); 6: tsw_stats coop_worker_queries / coop_worker_pops;
 * 7: tsw_opts.reserved became host_astar, tsw_stats gained host_astar_queries / host_astar_used /
 * host_astar_ms, tsw_host_next_hop_codes; 8: tsw_nearby, tsw_decide_fleet. Still 8: tsw_fleet_apply and
 * tsw_fleet_run, and after them tsw_fleet_mapd, were added without touching a struct or an existing
 * signature, and so were tsw_audit_records and tsw_audit_records_device (one new struct, tsw_audit), and
 * then tsw_plan_mapd_online (no struct, no existing signature touched), and then tsw_task_timeline,
 * tsw_task_timeline_device and tsw_probe_timeline (one new struct, tsw_timeline), and then
 * tsw_astar_reserved, tsw_host_astar_reserved and tsw_probe_st_astar (two new structs, tsw_node_res and
 * tsw_edge_res); a
 * caller that wants them looks the symbols up (dlsym) instead of comparing the revision. */
#define TSW_ABI_VERSION 8

/* AgentState discriminants in declaration order (src/map/agent.rs:9-15) */
#define TSW_PICKING 0
#define TSW_CARRYING 1
#define TSW_DELIVERED 2
#define TSW_IDLE 3

/* Sentinel distance in tables: blocked or unreachable cell. */
#define TSW_DIST_INF 0xFFFFu

typedef struct tsw_ctx tsw_ctx;

/* src/map/map.rs:4 `pub type Point = (usize, usize)` */
typedef struct {
    uint32_t x, y;
} tsw_point;

/* src/map/task_generator.rs:6-12 `Task{pickup, delivery, peer_id, task_id}`;
 * peer_id/task_id are never read by the planner and are not carried. */
typedef struct {
    tsw_point pickup, delivery;
} tsw_task;

/* One element of tswap_mapd's Vec<Vec<(Point, AgentState)>> (tswap.rs:43). */
typedef struct {
    uint16_t x, y;
    uint8_t state; /* TSW_PICKING .. TSW_IDLE */
    uint8_t pad[3];
} tsw_rec;

/* Context options. Every option is results-neutral: plans, tables and next hops are bit-identical
 * whatever is set here; only time and memory change. The production library reads nothing from the
 * environment — these fields are its whole configuration surface. */
typedef struct {
    int32_t device;              /* HIP device ordinal (default 0)                                  */
    uint32_t flags;              /* TSW_F_* below                                                   */
    uint64_t table_budget_bytes; /* cap for detour-byte+next-hop tables, 2 B per cell per goal
                                    (0 = half of the device's free memory at tsw_create)            */
    uint32_t watchdog_ms;        /* plan calls: if the planner records no timestep for this long,
                                    the call finishes in exit mode (0 = 10000)                      */
    uint32_t host_astar;         /* coop mode: host threads answering the planner's needed A* pairs
                                    during the plan dispatch, the calling thread included (0 = 1;
                                    TSW_HOST_ASTAR_OFF = none; at most 16)                          */
} tsw_opts;

/* tsw_opts.host_astar: no host A* service (the K3 workers alone answer the planner). */
#define TSW_HOST_ASTAR_OFF 0xFFFFFFFFu

/* Resolve every multi-candidate next hop of every table eagerly (one big
 * batched A* pass right after the BFS tables) instead of lazily per step.
 * (default: eager when the grid has <= 4096 cells and the new tables hold <= 8M cells) */
#define TSW_F_EAGER_NEXTHOP 1u
/* Never eager (lazy only), even when the auto policy would pick eager. */
#define TSW_F_LAZY_NEXTHOP 2u
/* Lazy next hops without concurrent K3 workers: the plan kernel exits to the host whenever a step
 * needs unresolved next hops and is relaunched after a batched A* pass ("exit mode"). Default
 * (coop mode): the plan dispatch also runs exact-A* worker waves on the other CUs, which the planner
 * feeds through device queues and waits on only when a step needs a code. */
#define TSW_F_EXIT_MODE 4u

/* Replaces the graph build of tswap_mapd (tswap.rs:44-77) and of the
 * centralized manager (bin/centralized/manager.rs:503-535): uploads the grid
 * and builds the device neighbour masks. cells: h rows of w bytes.
 * opts may be NULL. Returns NULL on failure (see tsw_last_error(NULL)). */
tsw_ctx *tsw_create(const uint8_t *cells, uint32_t w, uint32_t h, const tsw_opts *opts);
void tsw_destroy(tsw_ctx *ctx);
/* Message of the last failure on ctx (ctx may be NULL: last create failure). */
const char *tsw_last_error(const tsw_ctx *ctx);
/* TSW_ABI_VERSION the library was built with; compare it with the header's before tsw_create. */
int tsw_abi_version(void);
/* Provenance of the build: the first 8 bytes of the sha1 of the library's sources (kernels, host
 * runtime, this header) as computed by the build, 0 if the build did not set it. Measurement tools
 * record it beside a profile and refuse to pair a profile with a different build. */
uint64_t tsw_build_id(void);

/* Replaces `tswap_mapd(grid, initial_positions, tasks)` (tswap.rs:39-172).
 * out: caller-allocated n*(max_t+1) records, agent-major:
 *   out[i*(max_t+1) + t] == paths[i][t]  for t < *out_T.
 * max_t = 2000 reproduces the reference's `timestep > 2000` stop (:167).
 * Returns TSW_EINVAL where the reference panics: a start off-grid or blocked
 * (checked up front, :94), a task whose off-grid/blocked pickup gets assigned
 * (:136), or whose off-grid/blocked delivery is looked up when its agent reaches
 * the pickup (:112). A bad task cell that is never looked up does not fail the
 * call. The nearest-pickup choice uses the raw pickup point (:125-130), its
 * coordinates clamped to 0xFFFE (cannot change the winner: see plan_impl, tsw_plan_host.hip). */
int tsw_plan_mapd(tsw_ctx *ctx, const tsw_point *starts, uint32_t n, const tsw_task *tasks,
                  uint32_t m, uint32_t max_t, tsw_rec *out, uint32_t *out_T);

/* As tsw_plan_mapd, additionally writing the goal cell id of every agent after
 * each step (same layout as out) — a debug trace for parity localisation.
 * goal_out may be NULL. */
int tsw_plan_mapd_trace(tsw_ctx *ctx, const tsw_point *starts, uint32_t n, const tsw_task *tasks,
                        uint32_t m, uint32_t max_t, tsw_rec *out, uint32_t *goal_out,
                        uint32_t *out_T);

/* Online MAPD: tswap_mapd (tswap.rs:39-172) with a release time per task. release[k] is the first
 * iteration that sees task k; release == NULL means every task is released at 0. Two changes to the loop:
 *   1. Visibility. Iteration t is the one that produces column t. Its nearest-pickup scan (:123-131)
 *      skips every task k with release[k] > t. Among the visible unused tasks the choice is unchanged:
 *      minimum Manhattan distance to the raw pickup point, lowest task index on ties. Release times do
 *      not reorder tasks.
 *   2. Termination (:163-169). The run ends after recording column t when every task is used (a task
 *      not yet released is not used) and every agent is idle, or when t + 1 > max_t. A fleet that is idle
 *      while tasks are still to come keeps producing columns: tswap_step still runs, so an idle agent that
 *      a goal swap sent elsewhere walks on; once every agent rests on its goal the columns repeat
 *      (state TSW_IDLE).
 * So: release all zero (or NULL) gives exactly tsw_plan_mapd_trace's output; a task with release > max_t
 * is never seen, and the run then ends at max_t with *out_T = max_t + 1; task cells are looked up lazily
 * as in tsw_plan_mapd (a bad pickup fails the call with TSW_EINVAL when it is assigned, a bad delivery
 * when its agent reaches the pickup, a bad task that is never released never). Everything else is
 * tsw_plan_mapd_trace's: the record layout, goal_out (may be NULL), max_t <= 2^20, the argument checks,
 * the refusal of re-entry from a resolver. */
int tsw_plan_mapd_online(tsw_ctx *ctx, const tsw_point *starts, uint32_t n, const tsw_task *tasks,
                         const uint32_t *release, uint32_t m, uint32_t max_t, tsw_rec *out,
                         uint32_t *goal_out, uint32_t *out_T);

/* Caller-resolved K3 (the per-step query batch sharded by goal owner, the
 * answers gathered). tsw_plan_mapd_resolved plans like tsw_plan_mapd_trace, in exit mode (no K3
 * workers in the plan dispatch), and hands every batch of (start, goal) cell pairs a step needs
 * — plus the speculative pairs queued with it — to `resolve` instead of running the exact A*
 * itself. resolve must fill code[i] with the next-hop code of get_path(start[i], goal[i]) (0..3
 * = S,E,N,W neighbour, tswap.rs:62 order; 4 = stay), e.g. by sending each pair to the rank that
 * owns its goal (tsw_next_hop_codes there) and gathering the codes, and return 0; anything else,
 * or a code > 4, fails the call with TSW_EINVAL. The plan is bit-identical to tsw_plan_mapd's.
 * The resolver must not call back into `ctx` (the suspended plan owns its queues and table store):
 * every entry point returns TSW_EINVAL on a context whose resolver is running. Answer the pairs
 * from another context (e.g. the goal owner's, tsw_next_hop_codes there). */
typedef int (*tsw_resolve_fn)(void *user, uint32_t k, const uint32_t *start, const uint32_t *goal, uint8_t *code);
int tsw_plan_mapd_resolved(tsw_ctx *ctx, const tsw_point *starts, uint32_t n, const tsw_task *tasks,
                           uint32_t m, uint32_t max_t, tsw_rec *out, uint32_t *goal_out, uint32_t *out_T,
                           tsw_resolve_fn resolve, void *user);

/* Next-hop codes of get_path(start[i], goal[i]) (tswap.rs:288-390) as tsw_plan_mapd_resolved's
 * resolver returns them (0..3 S,E,N,W, 4 = stay), served from this context's table store: new
 * goals get their K1 table, unresolved cells the exact A*, and both persist for later calls (a
 * goal owner's shard of the next-hop cache). */
int tsw_next_hop_codes(tsw_ctx *ctx, const uint32_t *start, const uint32_t *goal, uint32_t k, uint8_t *code);

/* The same codes from the host's exact A* alone — no context and no device: cells as tsw_create's
 * (h rows of w bytes), start[i] / goal[i] free cell ids (TSW_EINVAL otherwise). This is the search the
 * plan dispatch's host service runs (tsw_opts.host_astar): the BinaryHeap order, the S,E,N,W neighbour
 * order and the unreachable-goal fallback of get_path, so every code equals the device's. */
int tsw_host_next_hop_codes(const uint8_t *cells, uint32_t w, uint32_t h, const uint32_t *start,
                            const uint32_t *goal, uint32_t k, uint8_t *code);

/* Replaces one `tswap_step(&mut agents, &nodes)` call (tswap.rs:174-286;
 * per-tick copy in bin/centralized/manager.rs:147-259 via plan_all_paths
 * :101-144). v[i], g[i]: cell ids in/out, agent order = array order. */
int tsw_step(tsw_ctx *ctx, uint32_t *v, uint32_t *g, uint32_t n);

/* Batched `get_path(start, goal)` (tswap.rs:288-390), reduced to what every
 * caller consumes: next[q] = path[1] (start if len==1) and len[q] = len(path)
 * (1: start==goal, 2: unreachable fallback or adjacent goal, D+1 otherwise). */
int tsw_get_path_next(tsw_ctx *ctx, const uint32_t *start, const uint32_t *goal, uint32_t k,
                      uint32_t *next, int32_t *len);

/* Batched decentralized decision: compute_next_move_with_tswap
 * (src/bin/decentralized/agent.rs:329-462) for n agents, each with its own local view.
 * Agent i: cell my_v[i], goal my_g[i] (free cells, else TSW_EINVAL — the reference panics at
 * pos2id[&my_pos], :358); its nearby list is entries nb_off[i] .. nb_off[i+1]-1 of nb_v/nb_g
 * (the other agents' cell / goal cell ids in NearbyAgents::get_nearby order, self excluded,
 * :108-153; an id >= w*h or a blocked cell means "not on the map", :389-393).
 * Outputs per agent: act[i] = TSW_ACT_* (TswapAction, :321-326); cell[i] = Move destination
 * (the agent's own cell for Rule 1); partner[i] = list index of the goal-swap partner
 * (0xFFFFFFFF otherwise); npart[i] = number of rotation participants, whose list indices are
 * part[nb_off[i] + i .. + npart[i]) (part holds nb_off[n] + n entries). */
#define TSW_ACT_MOVE 0u
#define TSW_ACT_GOAL_SWAP 1u
#define TSW_ACT_ROTATION 2u
#define TSW_ACT_WAIT 3u
int tsw_decide(tsw_ctx *ctx, const uint32_t *my_v, const uint32_t *my_g, uint32_t n, const uint32_t *nb_off,
               const uint32_t *nb_v, const uint32_t *nb_g, uint32_t *act, uint32_t *cell, uint32_t *partner,
               uint32_t *npart, uint32_t *part);

/* K5: NearbyAgents::get_nearby (agent.rs:108-153) for a whole fleet. v[i] = cell id of agent i
 * (any on-grid cell; TSW_EINVAL for an id >= w*h). Agent i's list is every agent j != i with
 * |xi-xj| + |yi-yj| <= radius (obstacles play no part; agents sharing i's cell are included; self is
 * excluded by index), in ASCENDING AGENT INDEX. The reference's list order is a HashMap iteration
 * order, i.e. unspecified; ascending agent index is this library's deterministic choice. A decision
 * depends on the order only through "first entry at a position", which this order makes the
 * smallest-index agent at the cell. nb_off[n+1] is always written; *total = nb_off[n].
 * nb_idx (agent indices, CSR) is written only when *total <= cap; otherwise TSW_EOVERFLOW with nb_off
 * and *total valid (nb_idx may be NULL with cap 0: a size query). n == 0: TSW_OK with nb_off[0] = 0.
 * Duplicate positions are legal (in the decentralized mode they stand for stale information). */
int tsw_nearby(tsw_ctx *ctx, const uint32_t *v, uint32_t n, uint32_t radius,
               uint32_t *nb_off, uint32_t *nb_idx, uint32_t cap, uint32_t *total);

/* One decentralized tick for the fleet: the lists of tsw_nearby, then compute_next_move_with_tswap for
 * every agent, all on the device (the lists never visit the host). Defined as: the outputs of
 * tsw_decide(my_v = v, my_g = g, lists nb_v[k] = v[nb_idx[k]], nb_g[k] = g[nb_idx[k]]) with every list
 * index replaced by the agent index it names. act/cell as tsw_decide; partner[i] = AGENT index or
 * 0xFFFFFFFF; rotation participants as agent indices in part[part_off[i] .. part_off[i+1]) (empty
 * unless act[i] == TSW_ACT_ROTATION). part_off[n] > part_cap: TSW_EOVERFLOW with act, cell, partner,
 * part_off complete and part untouched. Errors as tsw_decide: a v[i] or g[i] off-grid or blocked is
 * TSW_EINVAL; a list of more than 1024 entries that reaches Rule 4 is TSW_EOVERFLOW (part_off[n] is
 * then not written). n == 0: TSW_OK with part_off[0] = 0. */
int tsw_decide_fleet(tsw_ctx *ctx, const uint32_t *v, const uint32_t *g, uint32_t n, uint32_t radius,
                     uint32_t *act, uint32_t *cell, uint32_t *partner,
                     uint32_t *part_off, uint32_t *part, uint32_t part_cap);

/* The decentralized mode in lock step. The reference's agents gossip asynchronously; the transport is
 * not modelled. What is modelled is the effect of the timer branch (bin/decentralized/agent.rs:838-927)
 * and of the message handlers it triggers, under one deterministic schedule:
 *   - in one TICK every agent runs the timer branch once, on fresh information: everyone's broadcast
 *     position and goal are the tick-start arrays v0, g0;
 *   - each agent's outgoing messages are delivered and handled before the next agent's turn;
 *   - agents take their turns in ASCENDING AGENT INDEX (the choice already made for the list order).
 * With (act, cell, partner, part_off, part) = tsw_decide_fleet(v0, g0, radius) and G a copy of g0, for
 * i = 0 .. n-1 in order:
 *   TSW_ACT_MOVE (:854-857)       v1[i] = cell[i]. No collision check, as in the reference: two agents
 *                                 may enter one cell (duplicate positions are legal inputs). Moves read
 *                                 v0 only, so their order plays no part.
 *   TSW_ACT_GOAL_SWAP, j = partner[i]
 *                                 (request :892-905, the partner's handler :1041-1072, the response
 *                                 :1075-1087) the partner takes the requester's goal and answers with
 *                                 the goal it held: G[i] and G[j] are exchanged, at their values of turn i.
 *   TSW_ACT_ROTATION, P = part[part_off[i] .. part_off[i+1]), k = |P|
 *                                 (request :907-920, handler :1090-1107) for m = 0 .. k-1:
 *                                 G[P[m]] = g0[P[(m+1) % k]]. The request carries the goals of the
 *                                 initiator's nearby information, i.e. the tick-start g0, not G. As in
 *                                 the reference the initiator is not among its own participants and
 *                                 keeps its goal.
 *   TSW_ACT_WAIT                  nothing.
 * Every other v1[i] = v0[i]; g1 = G. Left out — the caller's business between calls: the agent's
 * bookkeeping (pending_goal_swap is always cleared within the tick; pending_rotation is never cleared
 * in the reference), task_state, my_task and the pickup / delivery hand-over (tsw_fleet_mapd, below,
 * runs the tick with a task phase of this library's own).
 *
 * tsw_fleet_apply: one tick's decisions, in tsw_decide_fleet's output form (they may be the caller's
 * own), applied to v and g in place with exactly the sequential semantics above. TSW_EINVAL with v and g
 * untouched, checked on the host before anything is launched: an act > 3; a Move cell off-grid or
 * blocked; a swap partner >= n; a participant >= n; a rotation with fewer than 2 participants or one
 * that lists a participant twice; a part_off that is not non-decreasing. n == 0: TSW_OK. */
int tsw_fleet_apply(tsw_ctx *ctx, uint32_t *v, uint32_t *g, uint32_t n,
                    const uint32_t *act, const uint32_t *cell, const uint32_t *partner,
                    const uint32_t *part_off, const uint32_t *part);

/* Up to `ticks` ticks of the model with v and g resident on the device: per tick the lists, the decisions
 * (the tsw_decide_fleet pipeline) and their application; lists and decisions never visit the host.
 * v, g are checked as tsw_decide_fleet checks them (TSW_EINVAL for a cell or goal off-grid or blocked).
 * A tick is a pure function of (v, g), so a tick that changes neither is a fixed point: the run stops
 * there and that tick is not counted. *ticks_done = the number of ticks that changed something; on
 * return v and g hold the state after those ticks. v_rec / g_rec (each may be NULL): n * (ticks + 1)
 * words, agent-major like tsw_plan_mapd's out — v_rec[i*(ticks+1) + t] = agent i's cell after t ticks;
 * columns 0 .. *ticks_done are written, later columns are left untouched. ticks == 0: TSW_OK, column 0,
 * *ticks_done = 0. n == 0: TSW_OK, *ticks_done = 0. A tick that fails (TSW_EOVERFLOW: a list of more
 * than 1024 entries reaching Rule 4, or lists past 2^32 - 1 entries; TSW_ENOMEM; TSW_EHIP) returns its
 * code with v, g and *ticks_done describing the state before that tick; the context stays usable.
 * A run's goals stay inside the initial goal set (swaps permute goals, rotations copy g0 values) and its
 * positions on free cells (moves are next hops): the inputs are validated once for all ticks. */
int tsw_fleet_run(tsw_ctx *ctx, uint32_t *v, uint32_t *g, uint32_t n, uint32_t radius, uint32_t ticks,
                  uint32_t *v_rec, uint32_t *g_rec, uint32_t *ticks_done);

/* A MAPD run on the lock-step tick, resident on the device: tsw_plan_mapd's inputs and record layout,
 * the decentralized mode's movement. The model is this library's own composition of three pieces of the
 * reference, because the reference's decentralized hand-over cannot be reproduced: agent.rs:859-888 keys
 * pickup / delivery on the agent's OWN task cells, not on the goal it currently heads for, so after the
 * first goal swap or rotation the agent walks to another agent's goal, arrives at neither of its own
 * cells and its timer branch (:840) goes quiet for good; and task_state, once WaitingForGoalSwap /
 * WaitingForRotation (:904, :919), is never set back. Literally reproduced, the fleet freezes after its
 * first swap. Modelled instead:
 *   - the state and task management of tswap_mapd (algorithm/tswap.rs:106-121), keyed on v == g whatever
 *     goal the agent holds at the moment — the rule tsw_plan_mapd implements;
 *   - the dispatch of the decentralized manager (bin/decentralized/manager.rs:275-300, :526-551): an agent
 *     without a task gets the NEXT task of the stream; there is no nearest-pickup search;
 *   - the lock-step tick defined above tsw_fleet_apply.
 * State per agent i: v[i], g[i] (cell ids), st[i] in {IDLE, TO_PICKUP, TO_DELIVERY}, tk[i] (task index or
 * 0xFFFFFFFF); one counter `next`, the number of tasks handed out. Start: v[i] = g[i] = cell(starts[i]),
 * st = IDLE, tk = none, next = 0, t = 0. Then repeat:
 *   1. Task phase, for i = 0 .. n-1 in ascending index (tswap.rs:106-139 with the manager's dispatch in
 *      place of :125-131). If v[i] == g[i]: TO_PICKUP becomes TO_DELIVERY with g[i] =
 *      cell(tasks[tk[i]].delivery); TO_DELIVERY becomes IDLE with tk[i] = none. Then, if st[i] == IDLE and
 *      next < m: tk[i] = next, st[i] = TO_PICKUP, g[i] = cell(tasks[next].pickup), next += 1. An agent
 *      that goes idle takes a task in the same step; one just given a task is not checked for arrival
 *      again in that step.
 *   2. The tick: exactly one tick of the lock-step model on (v, g) with `radius` (tsw_decide_fleet followed
 *      by tsw_fleet_apply).
 *   3. Ending. done = (next == m and every st[i] == IDLE); unchanged = (stage 1 made no transition and the
 *      tick changed neither v nor g). If done: record column t, t += 1, end with *stalled = 0 — even when
 *      the step changed nothing, so m == 0 gives one column, as tswap_mapd does. Else if unchanged: a step
 *      is a pure function of the state, nothing will ever change again: end with *stalled = 1, this step is
 *      not recorded. Else: record column t, t += 1, and end with *stalled = 0 if t > max_t (tswap.rs:167).
 *   4. Record (tswap.rs:144-158): column t of agent i holds (x, y) of v[i] and the state TSW_IDLE for IDLE,
 *      TSW_PICKING for TO_PICKUP, and for TO_DELIVERY TSW_DELIVERED if v[i] == g[i], else TSW_CARRYING;
 *      g[i] in goal_out and tk[i] in task_out where those are given.
 * out, goal_out, task_out: agent-major, n * (max_t + 1) each, like tsw_plan_mapd_trace's; goal_out and
 * task_out may be NULL. Columns 0 .. *out_T - 1 are written, later columns are left untouched. stalled may
 * be NULL. TSW_EINVAL before anything is launched: a start off-grid or blocked; ANY task cell off-grid or
 * blocked — all m tasks are checked up front, dispatched or not: unlike tsw_plan_mapd there is no reference
 * panic site to imitate; max_t > 2^20; a NULL out_T, or a NULL out with n > 0. Duplicate starts are legal,
 * as everywhere in the fleet entry points. n == 0: TSW_OK, *out_T = 0, *stalled = 0. A step that fails
 * (tsw_fleet_run's codes: TSW_EOVERFLOW from the list limits, TSW_ENOMEM, TSW_EHIP) returns its code with
 * the columns before it written and counted in *out_T (TSW_EHIP: nothing is copied back and *out_T = 0);
 * the context stays usable. The goals of a run stay
 * inside starts + pickups + deliveries (task goals come from there, swaps permute, rotations copy
 * tick-start values): their tables are built once, before the first step (TSW_ENOMEM if the set does not
 * fit table_budget_bytes). */
int tsw_fleet_mapd(tsw_ctx *ctx, const tsw_point *starts, uint32_t n, const tsw_task *tasks, uint32_t m,
                   uint32_t radius, uint32_t max_t, tsw_rec *out, uint32_t *goal_out, uint32_t *task_out,
                   uint32_t *out_T, uint32_t *stalled);

/* K6: the audit of plan records, on the device. rec: n rows of records as every plan entry point writes
 * them (tsw_plan_mapd, tsw_fleet_mapd), agent-major: agent i's column t is rec[i*stride + t]; only columns
 * 0 .. T-1 are read and the pad bytes are ignored. The cell of a record is (x, y); a record is ON-GRID when
 * x < w && y < h; blocked cells are the context's grid's. Every quantity that looks at column t-1 is 0 in
 * column 0.
 * col (may be NULL): T * TSW_AUDIT_NCOL words, col[t*TSW_AUDIT_NCOL + k] =
 *   k 0-3  agents whose state is 0 .. 3 (TSW_PICKING .. TSW_IDLE)
 *   k 4    bad_state: agents with state > 3
 *   k 5    moved: agents whose (x, y) differs from column t-1
 *   k 6    deliveries: agents TSW_DELIVERED at t that were not at t-1 (at t = 0: TSW_DELIVERED)
 *   k 7    colocations: on-grid agents that are not the smallest index on their cell (= on-grid agents minus
 *          the distinct cells among them: the agents beyond the first on a cell)
 *   k 8    swaps: agents on-grid at t-1 and t that step from a to a 4-neighbour b while some other agent steps
 *          from b to a in the same transition. Agents are counted, not pairs; co-located agents that all take
 *          the edge all count.
 *   k 9    jumps: agents with |dx| + |dy| > 1 against column t-1 (coordinates only: diagonal steps, teleports)
 *   k 10   off_map: agents whose record is off-grid or on a blocked cell
 * agent (may be NULL): n * TSW_AUDIT_NAGENT words, agent[i*TSW_AUDIT_NAGENT + k] = 0 moves, 1 deliveries,
 *   2 columns in which i is charged with any violation kind, 3 the first such column (0xFFFFFFFF if none).
 * Violation kinds, the order of first_t / first_agent: 0 colocation, 1 swap, 2 jump, 3 off_map, 4 bad_state.
 * sum: the column sums and the first violations; computed whether or not col and agent are given.
 * moving_columns is what the bench line reports as moving timesteps.
 * TSW_EINVAL before anything is launched, the outputs untouched: a NULL sum; a NULL rec with n > 0 && T > 0;
 * stride < T; T > 2^20 + 1; a context inside its own resolver. n == 0 or T == 0: TSW_OK, an all-zero sum with
 * first_t / first_agent 0xFFFFFFFF, col and agent untouched. TSW_ENOMEM when the scratch does not fit (the
 * transpose alone is 4 B per record). The call reads the context's grid only: the table store, the queues
 * and the stats are untouched, and a plan after an audit equals a plan without one.
 * tsw_audit_records_device: the same with the records in DEVICE memory (e.g. a torch tensor's data_ptr on
 * the context's device), read in place with their stride; sum, col and agent are host memory in both forms. */
#define TSW_AUDIT_NCOL 11u   /* words per column in col[]   */
#define TSW_AUDIT_NAGENT 4u  /* words per agent in agent[]  */
#define TSW_AUDIT_NKIND 5u   /* violation kinds, above      */
typedef struct {
    uint64_t state_steps[4];   /* agent-columns per AgentState discriminant */
    uint64_t bad_state, moves, deliveries, colocations, swaps, jumps, off_map;
    uint32_t moving_columns;   /* columns t >= 1 with moves > 0 */
    uint32_t first_t[5];       /* per kind: smallest column with a violation, 0xFFFFFFFF if none */
    uint32_t first_agent[5];   /* smallest agent index charged with it in that column */
} tsw_audit;
int tsw_audit_records(tsw_ctx *ctx, const tsw_rec *rec, uint32_t n, uint32_t T, uint32_t stride,
                      tsw_audit *sum, uint32_t *col, uint32_t *agent);
int tsw_audit_records_device(tsw_ctx *ctx, const tsw_rec *dev_rec, uint32_t n, uint32_t T,
                             uint32_t stride, tsw_audit *sum, uint32_t *col, uint32_t *agent);

/* K8: the task timeline of plan records, on the device: which agent took each task, when it was assigned,
 * picked up and delivered — the figures of the reference's src/map/task_metrics.rs (TaskMetric: sent_time is
 * release, start_time is t_assign, completion_time is t_deliver, counted in steps). No plan entry point has to
 * report them: the records determine them. rec, n, T, stride: as tsw_audit_records (only columns 0 .. T-1 are
 * read, the pad bytes are ignored); any prefix of a run's columns is a valid input. starts, tasks, release, m:
 * what the plan call was given (release == NULL: every task is released at 0).
 * Internal states. S of a record is I for TSW_IDLE, P for TSW_PICKING, D for TSW_CARRYING or TSW_DELIVERED: the
 * Idle / ToPickup / ToDelivery of tswap_mapd (tswap.rs:106-121). S(i, -1) = I. The position of agent i before
 * iteration t is its (x, y) in column t-1, and starts[i] for t = 0 (a start coordinate above 0xFFFF is read
 * as 0xFFFF, the most a record holds).
 * Replay. Columns t = 0 .. T-1 in order, within a column the agents in ascending index; for agent i the
 * transition p = S(i, t-1) -> c = S(i, t):
 *   P->P, D->D        nothing
 *   P->D              the agent's task is carried from t: t_carry = t
 *   D->I, D->P        the agent's task is finished and the agent holds none; then dispatch
 *   I->I, I->P        dispatch
 *   P->I, I->D, or a record state > 3     inconsistency of kind 0
 * Dispatch for agent i at column t, rule TSW_TL_NEAREST: the candidates are the tasks k that are not taken and
 * have release[k] <= t. c = P with no candidate is an inconsistency of kind 1, c = I with a candidate one of
 * kind 2. c = P with candidates takes the k with the smallest |x - px| + |y - py| from the agent's position,
 * the lowest k on ties, where (px, py) is the raw pickup point with its coordinates clamped to 0xFFFE exactly
 * as tsw_plan_mapd clamps them. A take sets agent[k] = i and t_assign[k] = t. Rule TSW_TL_STREAM: the one
 * candidate is task `next` (0 at the start) while next < m, and a take is k = next++; kinds 1 and 2 alike;
 * release must be NULL, starts is not read and may be NULL.
 * Delivery. While agent i holds task k, the first column whose record is TSW_DELIVERED is t_deliver[k] (the
 * agent is freed in iteration t_deliver + 1).
 * "The agent's task" is the bookkeeping of agent_tasks[i] (tswap.rs:90, :134), as in the reference: TSWAP swaps
 * goals, so the cell an agent stands on at t_carry - 1 may be another task's pickup, and the delivery cell
 * another task's.
 * task (may be NULL: only the summary): m * TSW_TL_NTASK words, task[k*4 + 0 .. 3] = agent, t_assign, t_carry,
 * t_deliver; an event that did not happen is 0xFFFFFFFF. The replay stops at the first inconsistency in
 * (t, agent) order: then consistent = 0, bad_kind / bad_t / bad_agent name it, task[] and the sums hold exactly
 * the events strictly before that (t, agent), and the call still returns TSW_OK. Otherwise consistent = 1 and
 * the three bad fields are 0xFFFFFFFF. Records that contradict the dispatch rule are found this way: the
 * replay is an audit of the assignment.
 * sum: assigned, carried, delivered count the tasks that have the corresponding time; unreleased the tasks with
 * release > T - 1 (every task when T == 0); wait_sum is the sum of t_assign - release over the assigned tasks;
 * service_sum, service_min, service_max are over t_deliver - release of the delivered tasks (none delivered:
 * min 0xFFFFFFFF, max 0); carry_sum is the sum of t_deliver - t_carry; makespan the largest t_deliver
 * (0xFFFFFFFF if none).
 * TSW_EINVAL before anything is launched, the outputs untouched: a NULL sum; a NULL rec with n > 0 && T > 0; a
 * NULL tasks with m > 0; a NULL starts with rule TSW_TL_NEAREST and n > 0 && T > 0; stride < T; T > 2^20 + 1;
 * rule > 1; release != NULL with TSW_TL_STREAM; a context inside its own resolver. n == 0 or T == 0: TSW_OK
 * with consistent = 1, nothing assigned, every task[] word 0xFFFFFFFF and unreleased as defined. TSW_ENOMEM
 * when the scratch does not fit (one byte per record and 36 bytes per task). Like the audit the call reads no
 * table and touches neither the table store, the queues nor the stats: a plan after a timeline equals a plan
 * without one.
 * tsw_task_timeline_device: the same with the records in DEVICE memory, read in place with their stride;
 * every other argument is host memory in both forms. */
#define TSW_TL_NEAREST 0u  /* tswap_mapd's dispatch (tswap.rs:123-137), with tsw_plan_mapd_online's visibility */
#define TSW_TL_STREAM 1u  /* tsw_fleet_mapd's dispatch: the next task of the stream */
#define TSW_TL_NTASK 4u  /* words per task in task[] */
typedef struct {
    uint64_t wait_sum, service_sum, carry_sum;
    uint32_t assigned, carried, delivered, unreleased;
    uint32_t service_min, service_max, makespan;
    uint32_t consistent, bad_kind, bad_t, bad_agent;
} tsw_timeline;
int tsw_task_timeline(tsw_ctx *ctx, const tsw_rec *rec, uint32_t n, uint32_t T, uint32_t stride,
                      const tsw_point *starts, const tsw_task *tasks, const uint32_t *release, uint32_t m,
                      uint32_t rule, tsw_timeline *sum, uint32_t *task);
int tsw_task_timeline_device(tsw_ctx *ctx, const tsw_rec *dev_rec, uint32_t n, uint32_t T, uint32_t stride,
                             const tsw_point *starts, const tsw_task *tasks, const uint32_t *release,
                             uint32_t m, uint32_t rule, tsw_timeline *sum, uint32_t *task);
/* Measurement probe (not part of the reference interface): the last timeline call of the context. out[0..2] =
 * ms of the passes A (events), B (replay) and C (attach), HIP-event timed on the context stream (0 with timing
 * off); out[3] = takes replayed; out[4] = candidates scanned by the takes' arg-min, summed. */
int tsw_probe_timeline(const tsw_ctx *ctx, double *out);

/* K9: astar_with_reservation (src/algorithm/a_star.rs:32-112), batched: k space-time A* searches over
 * (cell, time) with WAIT moves that avoid reserved vertices (cell, t) and edges ((from, to), t). Query i is
 * (start[i], goal[i], start_time[i]), cell ids of free cells. This is the primitive only: a prioritised planner
 * (agents in sequence, each reserving its path) is not in the reference and not in this library.
 * Search. The open set is a BinaryHeap of TimeNode {pos, g, f}, g the time, f = g + Manhattan(pos, goal), ordered
 * by a_star.rs:15-19 (smaller f first, then smaller g; pos takes no part) — AstarNode's order, restated once
 * for the whole library. (start, start_time) is pushed first and is not checked against the reservations. A
 * popped node at the goal ends the search: the path is its came_from chain. Otherwise its successors are
 * generated in the order (dx, dy) = (1,0), (-1,0), (0,1), (0,-1), (0,0) — x the column, y the row, the last
 * one WAIT — with np the successor cell and nt = g + 1, and one is skipped when
 *   np is off the grid or blocked ('@'), or (np, nt) is a reserved vertex, or (pos, nt) is a reserved vertex
 *   (a reserved current cell forbids leaving it too: the reference's rule), or ((pos, np), nt) or ((np, pos), nt)
 *   is a reserved edge (WAIT: ((pos, pos), nt)), or the state (np, nt) was pushed before;
 * every other one records came_from[(np, nt)] = (pos, g) and is pushed. Every state is pushed at most once.
 * Where the reference is replaced. (1) It bounds the grid by its compile-time 100 x 100 and takes every byte
 * but '.' as blocked; here the bounds are the context's w, h and blocked is '@' — identical on maps of '.' and
 * '@'. (2) It never returns when the goal cannot be reached (WAIT makes the state space infinite). Two caps,
 * both at points where they cannot change a path that is found: a popped node with f > max_time stops the
 * search with TSW_SP_NONE (pushes are never filtered by time, so the heap — and the tie-break — is the
 * reference's up to that pop, and any path that arrives by max_time is the reference's); a push that would be
 * the (max_nodes + 1)-th of the query, the start included, stops it with TSW_SP_CAPACITY. An emptied heap (the
 * start boxed in) is the reference's None: TSW_SP_NONE.
 * Outputs, CSR: query i's path is path[path_off[i] .. path_off[i+1]) as cell ids, entry j the cell at time
 * start_time[i] + j, the first one start[i]; empty unless status[i] == TSW_SP_FOUND. path_off[k+1] and *total =
 * path_off[k] are always written. *total > path_cap: TSW_EOVERFLOW with path_off, status, pops and *total valid
 * and path untouched (path may be NULL with path_cap 0: a size query). pops (may be NULL): pops[i] = nodes
 * popped with f <= max_time, the goal's pop included.
 * TSW_EINVAL before anything is launched, the outputs untouched: a start or goal off the grid or blocked;
 * max_time > 2^20; a start_time[i] > 2^20; max_nodes == 0; a NULL array whose count is not 0 (start, goal,
 * start_time, path_off, status, total with k > 0; node_res / edge_res with n_node / n_edge > 0; path with
 * path_cap > 0); a context inside its own resolver. start_time[i] + Manhattan > max_time is no error:
 * TSW_SP_NONE with 0 pops. Reservation entries may repeat and may name off-grid cells, non-adjacent pairs or
 * times past the horizon: legal, never matched. k == 0: TSW_OK with path_off[0] = 0 and *total = 0. TSW_ENOMEM
 * when the scratch of even one query does not fit (8 bytes per visited-table slot, 2 * max_nodes slots
 * rounded up to a power of two, and 8 bytes per node of the overflow heap, max_nodes taken as at most
 * w * h * (max_time + 2), the number of states a search can push); otherwise the queries run
 * in as many batches as the free memory needs. A reservation list of more than 2^30 keys, or a visited table of
 * more than 2^31 slots, is TSW_ENOMEM too. The scratch is grow-only and stays with the context until it is
 * destroyed: one table and one overflow heap per search wave in flight, at most min(k, 32 waves per CU) of
 * them and at most half of the free memory or 16 GiB — with the default max_nodes of 65,536 that is 1.5 MiB a
 * wave, 12 GiB for a call of 8,192 or more queries on a 256-CU device (wiped once, on the first call of that
 * size); a smaller max_nodes shrinks it in proportion. The call reads the grid only: the table store, the queues and
 * the stats stay as they were, and a plan after it equals a plan without it. */
typedef struct { uint32_t cell, t; } tsw_node_res;         /* (Point, time)            */
typedef struct { uint32_t from, to, t; } tsw_edge_res;     /* ((Point, Point), time)   */
#define TSW_SP_FOUND 0u
#define TSW_SP_NONE 1u
#define TSW_SP_CAPACITY 2u
int tsw_astar_reserved(tsw_ctx *ctx, const uint32_t *start, const uint32_t *goal, const uint32_t *start_time,
                       uint32_t k, const tsw_node_res *node_res, uint32_t n_node,
                       const tsw_edge_res *edge_res, uint32_t n_edge, uint32_t max_time, uint32_t max_nodes,
                       uint32_t *path_off, uint32_t *path, uint32_t path_cap, uint32_t *status,
                       uint32_t *pops, uint32_t *total);
/* The same search in plain C++ on the calling thread — no context and no device: cells as for the context's
 * creation (h rows of w bytes; TSW_EINVAL for a bad grid), every other argument and every output as above.
 * The serial form the device must equal and the CPU baseline it is measured against; it shares the reservation
 * set, the visited table and the heap order with the kernel, so the independent check of both is the test
 * suite's model. */
int tsw_host_astar_reserved(const uint8_t *cells, uint32_t w, uint32_t h, const uint32_t *start,
                            const uint32_t *goal, const uint32_t *start_time, uint32_t k,
                            const tsw_node_res *node_res, uint32_t n_node, const tsw_edge_res *edge_res,
                            uint32_t n_edge, uint32_t max_time, uint32_t max_nodes, uint32_t *path_off,
                            uint32_t *path, uint32_t path_cap, uint32_t *status, uint32_t *pops, uint32_t *total);
/* Measurement probe (not part of the reference interface): the last space-time A* call of the context, summed
 * over its batches, HIP-event timed on the context stream (0 with timing off). out[0] = ms of the reservation
 * set's build and upload, out[1] = ms of the search kernel, out[2] = ms of the path packing, out[3] = batches,
 * out[4] = search waves resident per batch. */
int tsw_probe_st_astar(const tsw_ctx *ctx, double *out);

/* K1: BFS distance tables for k goal cells, u16 per cell, row-major
 * (TSW_DIST_INF for blocked/unreachable). out: host buffer k*w*h. */
int tsw_dist_tables(tsw_ctx *ctx, const uint32_t *goals, uint32_t k, uint16_t *out);

/* K1 into caller-owned DEVICE memory (e.g. a torch tensor's data_ptr on the
 * context's device): dev_out receives k*w*h u16. Used for goal-sharded
 * construction + RCCL all-gather. */
int tsw_dist_tables_device(tsw_ctx *ctx, const uint32_t *goals, uint32_t k, uint16_t *dev_out);

/* Ingest k tables (k*w*h u16, DEVICE memory, e.g. the all-gather result)
 * into the context's table store so steps use them without recomputing. */
int tsw_import_tables_device(tsw_ctx *ctx, const uint32_t *goals, uint32_t k,
                             const uint16_t *dev_tables);

/* Next-hop codes of k goal tables (building them if needed), one byte per cell,
 * row-major: 0..3 = path[1] is the S,E,N,W neighbour (tswap.rs:62 order), 4 = stay
 * (unreachable goal, no closer neighbour), 0xFF = not resolved yet (lazy mode:
 * needs the exact A*). out: host buffer k*w*h. A goal held without a distance table
 * (u16 overflow, see the limits above) always comes back all 0xFF here, also with
 * TSW_F_EAGER_NEXTHOP: its next hops are resolved per query (tsw_get_path_next, plans),
 * never as a whole table; tsw_next_hop_tables_device returns TSW_EOVERFLOW for it. */
int tsw_next_hop_tables(tsw_ctx *ctx, const uint32_t *goals, uint32_t k, uint8_t *out);

/* Goal-sharded K3: the fully resolved next-hop codes of k goals into
 * caller-owned DEVICE memory (k*w*h bytes, row-major, codes as tsw_next_hop_tables). Builds the
 * goals' tables if needed and resolves every multi-candidate cell with the exact A* (eager,
 * whatever the context's next-hop policy): one rank's share of an all-gathered code table.
 * dev_dist (may be NULL): also receives the goals' K1 distance tables (k*w*h u16), so one K1 build
 * serves both all-gathers. */
int tsw_next_hop_tables_device(tsw_ctx *ctx, const uint32_t *goals, uint32_t k, uint8_t *dev_out,
                               uint16_t *dev_dist);

/* Ingest k tables AND their next-hop codes (DEVICE memory: k*w*h u16 + k*w*h u8, e.g. the
 * all-gather of tsw_dist_tables_device / tsw_next_hop_tables_device shards): steps then need
 * neither K1 nor K3 for those goals. Code 0xFF (or a pending marker) = not resolved here. */
int tsw_import_next_hops_device(tsw_ctx *ctx, const uint32_t *goals, uint32_t k, const uint16_t *dev_dist,
                                const uint8_t *dev_nh);

/* Drop every goal table and next-hop code held by the context (device memory
 * is kept for reuse). Later calls rebuild what they need. */
int tsw_clear_tables(tsw_ctx *ctx);

/* Per-context counters and kernel timings (HIP events on the context stream). */
typedef struct {
    uint64_t bfs_goals, bfs_launches;
    double bfs_ms;              /* summed K1 kernel time                     */
    uint64_t astar_queries, astar_launches;
    double astar_ms;            /* summed K3 kernel time                     */
    uint64_t walker_launches;   /* K2 serial-commit launches                 */
    double walker_ms;
    uint64_t assign_launches;
    double assign_ms;
    uint64_t steps;             /* timesteps planned                         */
    uint64_t tables;            /* goal tables resident                      */
    double plan_ms;             /* wall time of the last plan call           */
    /* inside the persistent plan kernel: device wall time per section, ms:
     * [0] assign [1] next-hop refresh [2] rules [3] refresh [4] movement
     * [5] record [6] done/other [7] launch copy-in/out */
    double plan_section_ms[8];
    uint64_t rule_rounds;       /* first-firing rounds run by the rules phase */
    /* plan-kernel exits for K3 next-hop resolution, by the section that needed the codes
     * (same indices as plan_section_ms; [7] = relaunch entry) */
    uint64_t plan_exits[8];
    uint64_t table_evictions;   /* goal tables dropped by the LRU (table_budget_bytes reached) */
    /* coop mode (K3 workers running concurrently with the planner): times the planner waited for
     * a worker, and its total waiting time (inside walker_ms) */
    uint64_t coop_waits;
    double coop_wait_ms;
    double coop_wait_sec_ms[8]; /* ... by planner section (plan_section_ms indices) */
    uint64_t coop_waits_sec[8];
    /* rules-phase cycle relabels: block-wide pointer doubling / incremental walks */
    uint64_t relabels_full, relabels_inc;
    uint64_t move_rounds;       /* decidability rounds run by the movement phase */
    uint32_t plan_block;        /* workgroup size of the last plan kernel launch */
    uint32_t coop_workers;      /* K3 worker waves in the last coop plan dispatch */
    /* coop mode: wall time the workers spent inside A*, summed over worker waves (wave-ms), by queue:
     * [0] needed pairs, [1] speculative prefetches, [2] task chains */
    double coop_worker_busy_ms[3];
    uint64_t watchdog_fires;    /* plan calls the host watchdog moved to exit mode */
    uint64_t tableless_goals;   /* goals held without a distance table (u16 overflow; next hops by K3) */
    /* coop mode (ABI 6): A* queries the workers ran and the heap pops they took, by queue (as
     * coop_worker_busy_ms): busy / pops = the in-dispatch time per pop */
    uint64_t coop_worker_queries[3];
    uint64_t coop_worker_pops[3];
    /* coop mode (ABI 7), host A* service: needed pairs the host answered, codes the planner took from
     * a host reply (the others arrived from a K3 worker first), and the host's time inside the A* */
    uint64_t host_astar_queries;
    uint64_t host_astar_used;
    double host_astar_ms;
} tsw_stats;
int tsw_get_stats(const tsw_ctx *ctx, tsw_stats *out);
int tsw_reset_stats(tsw_ctx *ctx);
/* Enable/disable HIP-event timing around kernels (default on). */
int tsw_set_timing(tsw_ctx *ctx, int enabled);
/* Measurement probe (not part of the reference interface): latency floors of the plan kernel's
 * round shapes on a `block`-thread workgroup (0 = the last plan's), HIP-event timed on the context
 * stream. out[0] = us per wave-0 rules firing chain (LDS load of 64 candidates, ballot, first lane,
 * readlane, that lane's store), out[1] = us per block-wide pass (LDS exchange + barrier; a movement
 * round is three). bench.py reports k_plan against rule_rounds * out[0] + 3 * move_rounds * out[1]. */
int tsw_probe_round_floors(tsw_ctx *ctx, uint32_t block, double *out);

#ifdef __cplusplus
}
#endif
#endif
