// stream_plan.h -- which HIP streams the stream pipeline (mpa_map_batches) creates, in which priority class and in which order, for the
// number of hardware queues the process has.  Host only: no HIP, no context, no globals (like dp_plan.h); dev_ctx.hip creates what the
// plan says, tests/stream_plan_check.cpp pins the policy without a device.
//
// The model behind it (measured in profiles/hw_queues_ab.txt): the runtime keeps one pool of at most Q =
// GPU_MAX_HW_QUEUES hardware queues PER PRIORITY CLASS and gives a new stream the least-used queue of its class, so the first Q streams
// created in a class get a queue each and the k-th sits on queue slot k mod Q of that class as far as the counts go (which of several
// equally used queues a later stream gets is the runtime's choice).  Everything on one queue runs in order: a copy or a microsecond
// kernel of one stream waits for whatever long kernel another stream has on the same queue.  Not in the plan: the process's null
// stream, which holds a queue of the normal class once something has used it.
#ifndef MPA_STREAM_PLAN_H
#define MPA_STREAM_PLAN_H
#include <cstdint>

namespace mpa {

enum StreamClass : int32_t { SC_NORMAL = 0, SC_HIGH = 1, SC_LOW = 2 };
// SL_LEGACY: every context a normal main stream, seeders and planners a high seed stream on first use, up to 16 normal side streams per
// lane.  The others give a seeder or planner ONE stream and cap the side streams:
//   SL_A  lanes normal, those beyond Q high; seeders high; planners and side streams low
//   SL_B  lanes normal, those beyond Q high; seeders high; planners normal, behind the lanes; side streams low
//   SL_C  the legacy classes: lanes normal (all of them), seeders and planners high; side streams normal while a queue is free there, else low
enum StreamLayout : int32_t { SL_LEGACY = 0, SL_A = 1, SL_B = 2, SL_C = 3 };

struct StreamSlot { int32_t cls, rank; };        // priority class; position in creation order over all streams of the plan
struct StreamPlan {
	static const int kMaxLanes = 8, kMaxSeed = 4, kMaxPlan = 6, kMaxSide = 16;   // (mpa_ctx_s::kSide; a round uses at most fifteen, its last event pair times the round)
	int32_t q, n_lanes, n_seed, n_plan;
	int32_t layout;                              // the layout in force: SL_LEGACY also where q covers every busy stream
	int32_t n_streams;                           // streams created up front (side streams come on first use)
	StreamSlot lane[kMaxLanes];
	int32_t side_cap[kMaxLanes], side_cls[kMaxLanes];   // side streams a lane may create (0: its launches take the lane's own stream) and their class
	StreamSlot seed_main[kMaxSeed], seed_seed[kMaxSeed];   // a seeder's main stream and its seeding stream: the same slot unless SL_LEGACY
	StreamSlot plan_main[kMaxPlan], plan_seed[kMaxPlan];   // a planner's, likewise
};

// q: GPU_MAX_HW_QUEUES as the process sees it (clamped to 1 .. 32); the counts are clamped to the pipeline's own limits.
// q >= n_lanes + n_seed + n_plan gives SL_LEGACY whatever was asked for.
StreamPlan stream_plan(int q, int n_lanes, int n_seed, int n_plan, int layout);

// the plan as int32 words (mpa_dbg_stream_plan): q, lanes, seeders, planners, layout, n_streams; per lane cls, rank, side_cap, side_cls;
// per seeder and then per planner main cls, main rank, seed cls, seed rank.  Returns the words it takes (written when they fit cap).
int64_t stream_plan_words(const StreamPlan &p, int32_t *out, int64_t cap);

// MPA_STREAM_PLAN as a layout: unset, empty or "1" the default, "0" SL_LEGACY, "A" / "B" / "C" that layout
int stream_layout_of(const char *env);
const int kStreamLayoutDefault = SL_A;

} // namespace mpa
#endif
