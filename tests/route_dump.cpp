// route_dump.cpp -- prints which kernels launch_chain_dp would take over a table of calls (tests/test_cpu_route.py compares the output with
// tests/golden/route_table.txt).  Every call is a dry run: no HIP call is made and no pointer is followed, so no device is needed and (T *)16 stands for
// "this array is there".  The output is the table's own format: the legend of the scalar sets and the variants, the distinct answers, then one line per case.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <vector>
#include "api_internal.h"

using mm2c::KParams;
using mm2c::LaunchArgs;

template <class T> static T *some() { return (T *)16; }

struct Scal { const char *name; std::function<void(KParams &)> set; };
struct Var { std::string name; std::function<void(LaunchArgs &)> set; };

static void dists(KParams &P, int x, int y) { P.max_dist_x = x; P.max_dist_y = y; P.max_dq = std::max(std::min(x, y), 0); }

static std::vector<Scal> scalar_sets()
{
	std::vector<Scal> S = {
		{"map-ont", [](KParams &) {}},
		{"max_skip=1023 max_iter=1024", [](KParams &P) { P.max_skip = 1023; P.max_iter = 1024; }},
		{"v2: max_skip=INT_MAX max_iter=1024", [](KParams &P) { P.max_skip = INT_MAX; P.max_iter = 1024; }},
		{"ava-ont: dist=10000 bw=2000", [](KParams &P) { dists(P, 10000, 10000); P.bw = 2000; }},
	};
	static const float gs[] = {0.5f, -0.5f, 19.5f, 20.f};
	static const int bws[] = {511, 512};
	static char gs_names[8][40];
	for (int g = 0; g < 4; ++g)
		for (int b = 0; b < 2; ++b) {
			char *nm = gs_names[g * 2 + b];
			snprintf(nm, 40, "gap_scale=%g bw=%d", gs[g], bws[b]);
			const float gv = gs[g]; const int bv = bws[b];
			S.push_back({nm, [gv, bv](KParams &P) { P.gap_scale = gv; P.bw = bv; }});
		}
	S.push_back({"bw=-1", [](KParams &P) { P.bw = -1; }});
	S.push_back({"max_dq-1<bw: dist_y=400", [](KParams &P) { dists(P, 5000, 400); }});
	S.push_back({"max_dist_x=65535", [](KParams &P) { dists(P, 65535, 5000); }});
	S.push_back({"max_dist_x=65536", [](KParams &P) { dists(P, 65536, 5000); }});
	S.push_back({"max_dq=32768", [](KParams &P) { dists(P, 32768, 32768); }});
	S.push_back({"max_dq=32769", [](KParams &P) { dists(P, 32769, 32769); }});
	static const int iters[] = {256, 257, 448, 449, 512, 513, 960, 961, 1024, 1025};
	static char it_names[10][24];
	for (int k = 0; k < 10; ++k) {
		snprintf(it_names[k], 24, "max_iter=%d", iters[k]);
		const int v = iters[k];
		S.push_back({it_names[k], [v](KParams &P) { P.max_iter = v; }});
	}
	S.push_back({"is_cdna", [](KParams &P) { P.is_cdna = 1; }});
	S.push_back({"n_segs=2", [](KParams &P) { P.n_segs = 2; }});
	S.push_back({"KF_FORCE_GENERAL", [](KParams &P) { P.flags |= mm2c::KF_FORCE_GENERAL; }});
	S.push_back({"KF_IGNORE_SEG", [](KParams &P) { P.flags |= mm2c::KF_IGNORE_SEG; }});
	// what decides whether a call whose max-skip exit cannot fire is given max_skip = max_iter - 1
	auto v2 = [](KParams &P) { P.max_skip = INT_MAX; P.max_iter = 1024; };
	S.push_back({"v2 gap_scale=0.5 bw=511", [v2](KParams &P) { v2(P); P.gap_scale = 0.5f; P.bw = 511; }});
	S.push_back({"v2 gap_scale=0.5 bw=512", [v2](KParams &P) { v2(P); P.gap_scale = 0.5f; P.bw = 512; }});
	S.push_back({"v2 bw=-1", [v2](KParams &P) { v2(P); P.bw = -1; }});
	S.push_back({"v2 max_dq-1<bw: dist_y=400", [v2](KParams &P) { v2(P); dists(P, 5000, 400); }});
	S.push_back({"v2 n_segs=2", [v2](KParams &P) { v2(P); P.n_segs = 2; }});
	S.push_back({"max_skip=0 max_iter=0", [](KParams &P) { P.max_skip = 0; P.max_iter = 0; }});
	return S;
}

// the call every variant departs from: a plan's -- class bytes, their counters, the packed words and the avg workspace are there, the knobs at their defaults
static LaunchArgs base_args()
{
	LaunchArgs L{};
	L.P.max_dist_x = 5000; L.P.max_dist_y = 5000; L.P.bw = 500; L.P.max_skip = 25; L.P.max_iter = 5000; L.P.is_cdna = 0; L.P.n_segs = 1;
	L.P.span_override = -1; L.P.max_dq = 5000; L.P.flags = 0; L.P.gap_scale = 1.0f;
	L.n_tasks = 8; L.d_offsets = some<const int64_t>(); L.d_anchors = some<const void>(); L.d_avg_ws = some<float>();
	L.d_cls = some<uint8_t>(); L.d_cls_stat = some<unsigned long long>(); L.d_w = some<int32_t>();
	L.d_f = some<int32_t>(); L.d_p = some<int32_t>(); L.d_t = some<int32_t>(); L.d_st = some<int32_t>(); L.d_status = some<int32_t>();
	L.far_ring = 1; L.max_task_anchors = 3000; L.dry_run = 1;
	return L;
}

static void host_out(LaunchArgs &L) { L.h_f = some<int32_t>(); L.h_p = some<int32_t>(); L.d_done = some<unsigned>(); L.h_flag = some<unsigned>(); L.seq = 1; }

static std::vector<Var> variants()
{
	std::vector<Var> V = {
		// knobs, one wave per task
		{"base", [](LaunchArgs &) {}},
		{"noskip_loop=0", [](LaunchArgs &L) { L.noskip_loop = 0; }},
		{"compact=0", [](LaunchArgs &L) { L.compact = 0; }},
		{"q24=0", [](LaunchArgs &L) { L.q24 = 0; }},
		{"q24=0 far_ring=2", [](LaunchArgs &L) { L.q24 = 0; L.far_ring = 2; }},
		{"packed_fp=0", [](LaunchArgs &L) { L.packed_fp = 0; }},
		{"no d_w", [](LaunchArgs &L) { L.d_w = nullptr; }},
		{"packed_fp=0 no d_w", [](LaunchArgs &L) { L.packed_fp = 0; L.d_w = nullptr; }},
		{"force_tab", [](LaunchArgs &L) { L.force_tab = 1; }},
		{"far_ring=0", [](LaunchArgs &L) { L.far_ring = 0; }},
		{"far_ring=2", [](LaunchArgs &L) { L.far_ring = 2; }},
		{"no d_cls", [](LaunchArgs &L) { L.d_cls = nullptr; }},
		{"no d_cls far_ring=0", [](LaunchArgs &L) { L.d_cls = nullptr; L.far_ring = 0; }},
		{"n_tasks=257", [](LaunchArgs &L) { L.n_tasks = 257; }},
		{"coop_waves=-1 (no cut)", [](LaunchArgs &L) { L.coop_waves = -1; }},
	};
	// the shape of a pass that asks for several waves per task
	auto coop = [&V](const std::string &name, std::function<void(LaunchArgs &)> set) {
		V.push_back({"coop_waves=16 " + name, [set](LaunchArgs &L) { L.coop_waves = 16; set(L); }});
	};
	for (int64_t nt : {8, 256, 257})
		for (int w8 : {256, 0})
			coop("n_tasks=" + std::to_string(nt) + " coop_w8_above=" + std::to_string(w8), [nt, w8](LaunchArgs &L) { L.n_tasks = nt; L.coop_w8_above = w8; });
	for (int64_t m : {(int64_t)0, (int64_t)7168, (int64_t)7169, ((int64_t)1 << 22) + 1})
		coop("max_task_anchors=" + std::to_string(m), [m](LaunchArgs &L) { L.max_task_anchors = m; });
	coop("st_ready", [](LaunchArgs &L) { L.st_ready = 1; });
	coop("st_ready d_avg", [](LaunchArgs &L) { L.st_ready = 1; L.d_avg = some<const float>(); });
	coop("fuse_st=0", [](LaunchArgs &L) { L.fuse_st = 0; });
	coop("fuse_st=0 st_ready d_avg", [](LaunchArgs &L) { L.fuse_st = 0; L.st_ready = 1; L.d_avg = some<const float>(); });
	coop("d_avg", [](LaunchArgs &L) { L.d_avg = some<const float>(); });
	coop("d_avg no d_avg_ws", [](LaunchArgs &L) { L.d_avg = some<const float>(); L.d_avg_ws = nullptr; });
	coop("no d_avg_ws", [](LaunchArgs &L) { L.d_avg_ws = nullptr; });
	coop("host out", [](LaunchArgs &L) { host_out(L); });
	coop("host out d_avg", [](LaunchArgs &L) { host_out(L); L.d_avg = some<const float>(); });
	coop("host out d_avg n_tasks=257", [](LaunchArgs &L) { host_out(L); L.d_avg = some<const float>(); L.n_tasks = 257; });
	coop("host out without h_flag", [](LaunchArgs &L) { host_out(L); L.h_flag = nullptr; });
	coop("host out without h_f", [](LaunchArgs &L) { host_out(L); L.h_f = nullptr; });
	coop("host out without h_p", [](LaunchArgs &L) { host_out(L); L.h_p = nullptr; });
	coop("host out without d_done", [](LaunchArgs &L) { host_out(L); L.d_done = nullptr; });
	coop("host out d_avg max_task_anchors=7169", [](LaunchArgs &L) { host_out(L); L.d_avg = some<const float>(); L.max_task_anchors = 7169; });
	coop("no d_cls", [](LaunchArgs &L) { L.d_cls = nullptr; });
	coop("long tasks: d_seg_ws", [](LaunchArgs &L) { L.d_seg_ws = some<unsigned long long>(); L.longest_task = 1 << 20; L.max_task_anchors = 1 << 20; });
	// what only the launches read (the prepass form, chain_cls_settle): the answer must not move with it
	V.push_back({"long tasks: d_seg_ws", [](LaunchArgs &L) { L.d_seg_ws = some<unsigned long long>(); L.longest_task = 1 << 20; L.max_task_anchors = 1 << 20; }});
	V.push_back({"no d_cls_stat", [](LaunchArgs &L) { L.d_cls_stat = nullptr; }});
	// the pairs that interact: a device-side cut with its count, class and distance arrays; per-task distances with and without them
	for (int coop_waves : {0, -1, 16})
		for (int bits = 0; bits < 8; ++bits)
			for (int td = 0; td < 2; ++td) {
				if (coop_waves == 16 && (bits & 3) != 3) continue;             // (asked for by the caller: refused by any cut, one form of it is enough)
				std::string name = "cut coop_waves=" + std::to_string(coop_waves) + ((bits & 1) ? " d_count" : "") + ((bits & 2) ? " cut.d_cls" : "") + ((bits & 4) ? " cut.d_dists" : "")
				                   + (td ? " d_task_dists" : "");
				V.push_back({name, [coop_waves, bits, td](LaunchArgs &L) {
					L.coop_waves = coop_waves; L.n_tasks = 256;
					L.cut.max_pieces = 300; L.cut.d_start = some<int64_t>(); L.cut.d_end = some<int64_t>(); L.cut.d_pbase = some<int32_t>(); L.cut.d_status = some<int32_t>();
					L.cut.d_has_cut = some<int32_t>(); L.cut.d_avg = some<float>();
					if (bits & 1) L.cut.d_count = some<int32_t>();
					if (bits & 2) L.cut.d_cls = some<uint8_t>();
					if (bits & 4) L.cut.d_dists = some<int32_t>();
					if (td) L.d_task_dists = some<const int32_t>();
				}});
			}
	for (int coop_waves : {0, -1})
		V.push_back({"cut coop_waves=" + std::to_string(coop_waves) + " d_count cut.d_cls, no d_cls", [coop_waves](LaunchArgs &L) {
			L.coop_waves = coop_waves; L.n_tasks = 256; L.d_cls = nullptr;
			L.cut.max_pieces = 300; L.cut.d_start = some<int64_t>(); L.cut.d_end = some<int64_t>(); L.cut.d_pbase = some<int32_t>(); L.cut.d_status = some<int32_t>();
			L.cut.d_has_cut = some<int32_t>(); L.cut.d_avg = some<float>(); L.cut.d_count = some<int32_t>(); L.cut.d_cls = some<uint8_t>();
		}});
	V.push_back({"d_task_dists", [](LaunchArgs &L) { L.d_task_dists = some<const int32_t>(); }});
	V.push_back({"d_task_dists coop_waves=16", [](LaunchArgs &L) { L.d_task_dists = some<const int32_t>(); L.coop_waves = 16; }});
	V.push_back({"d_task_dists no d_cls", [](LaunchArgs &L) { L.d_task_dists = some<const int32_t>(); L.d_cls = nullptr; }});
	return V;
}

int main()
{
	const std::vector<Scal> S = scalar_sets();
	const std::vector<Var> V = variants();
	std::map<std::string, int> index;
	std::vector<std::string> texts;
	std::string cases;
	for (size_t s = 0; s < S.size(); ++s)
		for (int rc = 0; rc <= 4; ++rc)
			for (size_t v = 0; v < V.size(); ++v) {
				LaunchArgs L = base_args();
				S[s].set(L.P); L.ring_class = rc; V[v].set(L);
				mm2c::LaunchInfo I = {};
				const hipError_t e = mm2c::launch_chain_dp(L, nullptr, nullptr, nullptr, &I);
				char var[256], line[400];
				mm2c_api::format_variant(I, var, sizeof var);
				snprintf(line, sizeof line, "rc=%d %s | host_out=%d single_ok=%d fused_st=%d route_auto=%d", (int)e, var, I.host_out, I.single_ok, I.fused_st, I.route_auto);
				auto it = index.find(line);
				if (it == index.end()) { it = index.emplace(line, (int)texts.size()).first; texts.push_back(line); }
				char key[64];
				snprintf(key, sizeof key, "%zu %d %zu %d\n", s, rc, v, it->second);
				cases += key;
			}
	printf("# scalar sets (departures from map-ont: dist 5000 / 5000, bw 500, max_skip 25, max_iter 5000, gap_scale 1)\n");
	for (size_t s = 0; s < S.size(); ++s) printf("S%zu %s\n", s, S[s].name);
	printf("# variants (departures from a plan's call of 8 tasks, longest 3000 anchors, one wave per task, far_ring 1, every workspace there, no d_avg, no cut)\n");
	for (size_t v = 0; v < V.size(); ++v) printf("V%zu %s\n", v, V[v].name.c_str());
	printf("# answers\n");
	for (size_t t = 0; t < texts.size(); ++t) printf("T%zu %s\n", t, texts[t].c_str());
	printf("# cases: scalar set, ring_class, variant, answer\n");
	fputs(cases.c_str(), stdout);
	return 0;
}
