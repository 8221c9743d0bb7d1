// phyamd_abi.inc -- the extern "C" entry points of include/physher_amd.h.
// (part of phyamd_engine.hip: one translation unit)
//
// A handle (`phyamd_engine`) is a GROUP of 1..n shards: shard s is a complete engine (phyamd_shard_api.inc) on its own GPU
// and stream that owns the contiguous pattern range [s P / n, (s+1) P / n) -- SURVEY 8e: patterns are independent given the
// tree and the parameters, tree / eigen system / rates are replicated (KBs), and the only cross-shard quantities are sums over
// patterns (lnL, the [node][category] gradient, parameter sums, root terms).  Every entry point below either
//   * replicates its arguments to all shards (tree, branch lengths, model),
//   * slices its per-pattern arguments (tip data, weights, per-pattern outputs), or
//   * runs an evaluation on all shards AT ONCE -- one host thread per shard, each driving its own device -- and adds the
//     per-shard result vectors on the host in shard order (fixed order: reproducible; 64 KB per shard at 1000 taxa x 4
//     categories, which the caller wants on the host anyway, so no device-side collective is involved in this single-process
//     form; the one-process-per-GPU form -- bench.py under torchrun -- uses ONE RCCL all-reduce of the same vector).
// A group of one shard makes the same calls inline, without threads.

#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

namespace {

// one persistent worker per shard (n > 1): a job is "run fn(shard index)", the caller waits for all of them
class ShardWorkers {
public:
	explicit ShardWorkers(int n) : done_(0), generation_(0), stop_(false) {
		for (int i = 0; i < n; i++) threads_.emplace_back([this, i] { loop(i); });
	}
	~ShardWorkers() {
		{
			std::lock_guard<std::mutex> lk(m_);
			stop_ = true;
			generation_++;
		}
		cv_.notify_all();
		for (auto &t : threads_) t.join();
	}
	// runs fn(i) for every shard i concurrently; returns when all have finished
	void run(const std::function<void(int)> &fn) {
		std::unique_lock<std::mutex> lk(m_);
		fn_ = &fn;
		done_ = 0;
		generation_++;
		cv_.notify_all();
		cv_done_.wait(lk, [this] { return done_ == (int)threads_.size(); });
		fn_ = nullptr;
	}

private:
	void loop(int i) {
		unsigned long seen = 0;
		for (;;) {
			const std::function<void(int)> *fn;
			{
				std::unique_lock<std::mutex> lk(m_);
				cv_.wait(lk, [&] { return generation_ != seen; });
				seen = generation_;
				if (stop_) return;
				fn = fn_;
			}
			(*fn)(i);
			{
				std::lock_guard<std::mutex> lk(m_);
				done_++;
			}
			cv_done_.notify_one();
		}
	}
	std::vector<std::thread> threads_;
	std::mutex m_;
	std::condition_variable cv_, cv_done_;
	const std::function<void(int)> *fn_ = nullptr;
	int done_;
	unsigned long generation_;
	bool stop_;
};

}  // namespace

struct phyamd_engine {
	std::vector<Shard *> shards;
	std::vector<int> offset;  // shard s owns patterns [offset[s], offset[s + 1])
	int T = 0, N = 0, P = 0, S = 0, C = 0;
	ShardWorkers *workers = nullptr;           // n > 1
	bool poisoned = false;                     // a replicated call failed on some shards only: their states differ, nothing can be summed
	std::vector<std::vector<double>> scratch;  // per-shard host result vectors
	std::vector<std::string> errors;
	double spr_ms = 0.0;                       // wall time of the last phyamd_spr_log_likelihoods
	double bhess_ms = 0.0;                     // wall time of the last phyamd_branch_hessian
};

namespace {

int group_size(const phyamd_engine *g) { return (int)g->shards.size(); }

// fn(shard, index) on every shard -- concurrently for n > 1 -- and the first failure (with its message) as the result
template <typename F>
int for_shards(phyamd_engine *g, F fn) {
	const int n = group_size(g);
	if (n == 1) return fn(g->shards[0], 0);
	std::vector<int> rc(n, PHYAMD_OK);
	const std::function<void(int)> job = [&](int i) {
		rc[i] = fn(g->shards[i], i);
		if (rc[i] != PHYAMD_OK) g->errors[i] = g_last_error;  // g_last_error is thread-local: hand the text to the caller
	};
	if (g->poisoned)
		return fail(PHYAMD_EINVAL, "an earlier call failed on some shards of this engine only (their states differ): destroy it and create a new one");
	g->workers->run(job);
	int failed = 0, first = -1;
	for (int i = 0; i < n; i++)
		if (rc[i] != PHYAMD_OK) {
			failed++;
			if (first < 0) first = i;
		}
	if (failed == 0) return PHYAMD_OK;
	// all shards refusing alike (a bad argument) leaves them in step; some of them failing (e.g. out of memory on one device) does not
	if (failed < n) g->poisoned = true;
	return fail(rc[first], "shard %d (device %d): %s", first, g->shards[first]->device, g->errors[first].c_str());
}

// per-shard vectors of `count` doubles -> their sum: pairwise up the bisection tree for 2, 4 or 8 shards (the shards ARE the
// subtrees of the bisection a single engine sums by, reduce_block_sums: the same additions in the same order, so the result does
// not depend on the shard count), in shard order otherwise
void sum_shards(const phyamd_engine *g, size_t count, double *out) {
	const int n = group_size(g);
	const bool tree = n == 2 || n == 4 || n == 8;
	for (size_t i = 0; i < count; i++) {
		if (tree) {
			double v[8];
			for (int s = 0; s < n; s++) v[s] = g->scratch[s][i];
			for (int m = n; m > 1; m >>= 1)
				for (int s = 0; s < m / 2; s++) v[s] = v[2 * s] + v[2 * s + 1];
			out[i] = v[0];
		} else {
			double v = g->scratch[0][i];
			for (int s = 1; s < n; s++) v += g->scratch[s][i];
			out[i] = v;
		}
	}
}

// shard boundaries in patterns.  2, 4 or 8 shards: the block range [0, ceil(P / 64)) bisected 1, 2 or 3 times (mid = lo + (hi - lo)
// / 2, the rule of reduce_block_sums), so that every shard is a subtree of the one-engine summation; otherwise equal parts.
void shard_offsets(int P, int n, std::vector<int> &offset) {
	offset.assign(n + 1, 0);
	if ((n == 2 || n == 4 || n == 8) && (P + WAVE - 1) / WAVE >= n) {
		std::vector<int> bounds;
		bisect_blocks(0, (P + WAVE - 1) / WAVE, n == 2 ? 1 : n == 4 ? 2 : 3, bounds);
		for (int s = 0; s < n; s++) offset[s] = bounds[s] * WAVE;
		offset[n] = P;
		return;
	}
	for (int s = 0; s <= n; s++) offset[s] = (int)((long long)s * P / n);
}

#define CHECK_GROUP(g) \
	if (!(g) || (g)->shards.empty()) return fail(PHYAMD_EINVAL, "null engine")
#define SINGLE_DEVICE_ONLY(g, what) \
	if (group_size(g) > 1) return fail(PHYAMD_EUNSUPPORTED, what " leaves its result on ONE device: not available on an engine sharded over several")

int create_group(const phyamd_config *cfg, int n, const int32_t *device_ids, phyamd_engine **out) {
	if (!cfg || !out) return fail(PHYAMD_EINVAL, "null argument");
	*out = nullptr;
	if (n < 1) return fail(PHYAMD_EINVAL, "device count must be >= 1 (got %d)", n);
	if (n > 1 && cfg->stream) return fail(PHYAMD_EINVAL, "a caller-owned stream belongs to one device: leave `stream` NULL for a sharded engine");
	if (n > 1 && cfg->pattern_count < n) return fail(PHYAMD_EINVAL, "%d patterns cannot be sharded over %d devices", cfg->pattern_count, n);
	int caller_device = -1;  // shard_create binds each shard's device: the caller's current device is put back
	(void)hipGetDevice(&caller_device);
	struct RestoreDevice {
		int d;
		~RestoreDevice() {
			if (d >= 0) (void)hipSetDevice(d);
		}
	} restore{n > 1 || device_ids ? caller_device : -1};
	phyamd_engine *g = new phyamd_engine();
	g->T = cfg->tip_count;
	g->N = 2 * cfg->tip_count - 1;
	g->P = cfg->pattern_count;
	g->S = cfg->state_count;
	g->C = cfg->category_count;
	shard_offsets(cfg->pattern_count, n, g->offset);  // physher_amd/sharding.py::shard_range
	const int levels = (n == 2 || n == 4 || n == 8) && (cfg->pattern_count + WAVE - 1) / WAVE >= n ? 3 - (n == 2 ? 1 : n == 4 ? 2 : 3) : 3;
	for (int s = 0; s < n; s++) {
		phyamd_config c = *cfg;
		c.pattern_count = g->offset[s + 1] - g->offset[s];
		if (n > 1 || device_ids) c.device = device_ids ? device_ids[s] : s;
		Shard *sh = nullptr;
		const int rc = shard_create(&c, &sh);
		if (rc != PHYAMD_OK) {
			for (Shard *x : g->shards) shard_destroy(x);
			delete g;
			return rc;
		}
		sh->reduce_levels = levels;
		g->shards.push_back(sh);
	}
	g->scratch.resize(n);
	g->errors.resize(n);
	if (n > 1) g->workers = new ShardWorkers(n);
	*out = g;
	return PHYAMD_OK;
}

void ensure_scratch(phyamd_engine *g, size_t count) {
	for (auto &v : g->scratch)
		if (v.size() < count) v.resize(count);
}

// fn(shard, index, out) leaves a shard's `count` doubles in out: one shard writes `total` itself, several write their scratch
// vectors at once and `total` is their sum (sum_shards).  What a shard masked in band the caller masks again by the summed lnL
template <typename F>
int sum_over_shards(phyamd_engine *g, size_t count, double *total, F fn) {
	if (group_size(g) == 1) return fn(g->shards[0], 0, total);
	ensure_scratch(g, count);
	int rc;
	if ((rc = for_shards(g, [&](Shard *s, int i) { return fn(s, i, g->scratch[i].data()); }))) return rc;
	sum_shards(g, count, total);
	return PHYAMD_OK;
}

// a packed vector [part | part | ...] into the caller's arrays, part by part (array, doubles); a null array's part is skipped
void unpack(const double *packed, std::initializer_list<std::pair<double *, size_t>> parts) {
	for (const auto &[to, count] : parts) {
		if (to) std::memcpy(to, packed, sizeof(double) * count);
		packed += count;
	}
}

// a batch on several shards: fn(shard, index, lnl [count], cat_gradient [count][N C] or null) into the shard's scratch vector,
// laid out [lnl | cat_gradient], and the sums unpacked into the caller's arrays
template <typename F>
int sum_batch_over_shards(phyamd_engine *g, int32_t count, double *lnl, double *cat_gradient, F fn) {
	const size_t ncat = (size_t)g->N * g->C, n = (size_t)count * (cat_gradient ? 1 + ncat : 1);
	std::vector<double> total(n);
	int rc;
	if ((rc = sum_over_shards(g, n, total.data(), [&](Shard *s, int i, double *v) { return fn(s, i, v, cat_gradient ? v + count : nullptr); }))) return rc;
	unpack(total.data(), {{lnl, (size_t)count}, {cat_gradient, (size_t)count * ncat}});
	return PHYAMD_OK;
}

// the wall time of a group-level call, into *ms when the call returns
struct WallTime {
	double *ms;
	std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
	~WallTime() { *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// the profile of a query call: the first shard's, the others' merged in by the call's own rule
template <typename Prof, typename Merge>
int merged_profile(phyamd_engine *g, Prof Shard::*slot, Prof *out, Merge merge) {
	CHECK_GROUP(g);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	*out = g->shards[0]->*slot;
	for (int i = 1; i < group_size(g); i++) merge(*out, g->shards[i]->*slot);
	return PHYAMD_OK;
}

}  // namespace

extern "C" {

const char *phyamd_last_error(void) { return g_last_error.c_str(); }
int phyamd_abi_version(void) { return PHYAMD_ABI_VERSION; }

int phyamd_create(const phyamd_config *cfg, phyamd_engine **out) { return create_group(cfg, 1, nullptr, out); }

int phyamd_create_sharded(const phyamd_config *cfg, int32_t device_count, const int32_t *device_ids, phyamd_engine **out) {
	return create_group(cfg, device_count, device_ids, out);
}

void phyamd_destroy(phyamd_engine *g) {
	if (!g) return;
	delete g->workers;  // joins
	for (Shard *s : g->shards) shard_destroy(s);
	delete g;
}

int phyamd_shard_count(phyamd_engine *g) {
	CHECK_GROUP(g);
	return group_size(g);
}

// --- per-pattern inputs: sliced ---------------------------------------------------------------------------------

int phyamd_set_tip_states(phyamd_engine *g, int tip, const uint8_t *states) {
	CHECK_GROUP(g);
	if (!states) return fail(PHYAMD_EINVAL, "null states");
	return for_shards(g, [&](Shard *s, int i) { return shard_set_tip_states(s, tip, states + g->offset[i]); });
}

int phyamd_set_tip_partials(phyamd_engine *g, int tip, const double *partials) {
	CHECK_GROUP(g);
	if (!partials) return fail(PHYAMD_EINVAL, "null partials");
	return for_shards(g, [&](Shard *s, int i) { return shard_set_tip_partials(s, tip, partials + (size_t)g->offset[i] * g->S); });
}

int phyamd_set_pattern_weights(phyamd_engine *g, const double *weights) {
	CHECK_GROUP(g);
	if (!weights) return fail(PHYAMD_EINVAL, "null weights");
	return for_shards(g, [&](Shard *s, int i) { return shard_set_pattern_weights(s, weights + g->offset[i]); });
}

int phyamd_compress_patterns(int device, int32_t taxon_count, int64_t site_count, const uint8_t *const *rows, const uint8_t *symbol_codes,
                             int32_t *pattern_count, uint8_t *patterns, double *weights) {
	return compress_patterns_device(device, taxon_count, site_count, rows, symbol_codes, pattern_count, patterns, weights);
}

// --- tree and model: replicated ---------------------------------------------------------------------------------

int phyamd_set_topology(phyamd_engine *g, const int32_t *left, const int32_t *right, int root) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_set_topology(s, left, right, root); });
}
int phyamd_set_branch_lengths(phyamd_engine *g, const double *lengths) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_set_branch_lengths(s, lengths); });
}
int phyamd_set_branch_length(phyamd_engine *g, int node, double length) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_set_branch_length(s, node, length); });
}
int phyamd_update_all_nodes(phyamd_engine *g) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_update_all_nodes(s); });
}
int phyamd_store(phyamd_engine *g) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_store(s); });
}
int phyamd_restore(phyamd_engine *g) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_restore(s); });
}
int phyamd_set_eigen(phyamd_engine *g, const double *eval, const double *evec, const double *ivec) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_set_eigen(s, eval, evec, ivec); });
}
int phyamd_set_frequencies(phyamd_engine *g, const double *freqs) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_set_frequencies(s, freqs); });
}
int phyamd_set_category_rates(phyamd_engine *g, const double *rates, const double *proportions) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_set_category_rates(s, rates, proportions); });
}
int phyamd_set_node_matrices(phyamd_engine *g, int node, const double *matrices) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_set_node_matrices(s, node, matrices); });
}
int phyamd_set_matrices(phyamd_engine *g, const double *matrices) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_set_matrices(s, matrices); });
}
int phyamd_set_rate_matrix(phyamd_engine *g, const double *Q) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_set_rate_matrix(s, Q); });
}
int phyamd_set_rate_matrix_derivatives(phyamd_engine *g, int count, const double *dQ) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_set_rate_matrix_derivatives(s, count, dQ); });
}
int phyamd_set_rescaling(phyamd_engine *g, int policy) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_set_rescaling(s, policy); });
}
int phyamd_set_keep_partials(phyamd_engine *g, int on) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_set_keep_partials(s, on); });
}
int phyamd_set_reduction_levels(phyamd_engine *g, int levels) {
	CHECK_GROUP(g);
	if (levels < 0 || levels > 3) return fail(PHYAMD_EINVAL, "reduction levels must be 0..3 (got %d)", levels);
	if (group_size(g) > 1) return fail(PHYAMD_EUNSUPPORTED, "a sharded engine sets its shards' reduction levels itself");
	g->shards[0]->reduce_levels = levels;
	return PHYAMD_OK;
}

int phyamd_set_profiling(phyamd_engine *g, int on) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_set_profiling(s, on); });
}
int phyamd_synchronize(phyamd_engine *g) {
	CHECK_GROUP(g);
	return for_shards(g, [&](Shard *s, int) { return shard_synchronize(s); });
}

// --- evaluation: all shards at once, per-shard sums added in shard order -----------------------------------------

int phyamd_log_likelihood(phyamd_engine *g, double *lnl) {
	CHECK_GROUP(g);
	if (!lnl) return fail(PHYAMD_EINVAL, "null lnl");
	return sum_over_shards(g, 1, lnl, [&](Shard *s, int, double *v) { return shard_log_likelihood(s, v); });
}

int phyamd_gradient(phyamd_engine *g, int flags, double *lnl, double *cat_gradient) {
	CHECK_GROUP(g);
	if (!cat_gradient) return fail(PHYAMD_EINVAL, "null cat_gradient");
	if (group_size(g) == 1) return shard_gradient(g->shards[0], flags, lnl, cat_gradient);
	const size_t n = (size_t)g->N * g->C;
	std::vector<double> total(1 + n);
	int rc;
	// a shard whose own lnL is NaN / inf hands back an all-NaN gradient (treelikelihood.c:327-332): the sums inherit it
	if ((rc = sum_over_shards(g, total.size(), total.data(), [&](Shard *s, int, double *v) { return shard_gradient(s, flags, v, v + 1); }))) return rc;
	unpack(total.data(), {{lnl, 1}, {cat_gradient, n}});
	return PHYAMD_OK;
}

int phyamd_branch_gradient(phyamd_engine *g, int flags, const double *rates_without_mu, double *lnl, double *branch_gradient) {
	CHECK_GROUP(g);
	if (!branch_gradient) return fail(PHYAMD_EINVAL, "null branch_gradient");
	std::vector<double> cg((size_t)g->N * g->C);
	int rc;
	if ((rc = phyamd_gradient(g, flags, lnl, cg.data()))) return rc;
	const Shard *e = g->shards[0];
	const double *r = rates_without_mu ? rates_without_mu : e->rates.data();
	for (int n = 0; n < g->N; n++) {  // gradient_branch_length_from_cat_inplace, treelikelihood.c:3129-3143
		if (g->C == 1) {
			branch_gradient[n] = cg[n];  // catCount == 1: no rate/weight factor (treelikelihood.c:3258-3266)
			continue;
		}
		double v = cg[(size_t)n * g->C] * e->props[0] * r[0];
		for (int c = 1; c < g->C; c++) v += cg[(size_t)n * g->C + c] * e->props[c] * r[c];
		branch_gradient[n] = v;
	}
	return PHYAMD_OK;
}

int phyamd_parameter_gradient(phyamd_engine *g, int flags, double *lnl, double *cat_gradient, double *parameter_gradient) {
	CHECK_GROUP(g);
	if (!parameter_gradient) return fail(PHYAMD_EINVAL, "null parameter_gradient");
	if (group_size(g) == 1) return shard_parameter_gradient(g->shards[0], flags, lnl, cat_gradient, parameter_gradient);
	const size_t ncat = (size_t)g->N * g->C, np = (size_t)g->shards[0]->np;
	std::vector<double> total(1 + ncat + np);
	int rc;
	if ((rc = sum_over_shards(g, total.size(), total.data(), [&](Shard *s, int, double *v) { return shard_parameter_gradient(s, flags, v, v + 1, v + 1 + ncat); }))) return rc;
	unpack(total.data(), {{lnl, 1}, {cat_gradient, ncat}, {parameter_gradient, np}});
	return PHYAMD_OK;
}

int phyamd_root_invariant_term(phyamd_engine *g, double *out) {
	CHECK_GROUP(g);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	return sum_over_shards(g, 1, out, [&](Shard *s, int, double *v) { return shard_root_invariant_term(s, v); });
}

int phyamd_root_frequency_term(phyamd_engine *g, double *out) {
	CHECK_GROUP(g);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	return sum_over_shards(g, (size_t)g->S, out, [&](Shard *s, int, double *v) { return shard_root_frequency_term(s, v); });
}

int phyamd_branch_log_likelihood(phyamd_engine *g, int node, double length, double *lnl, double *d1, double *d2) {
	CHECK_GROUP(g);
	if (group_size(g) == 1) return shard_branch_log_likelihood(g->shards[0], node, length, lnl, d1, d2);
	// lnL(t), its first and second derivative are sums over patterns, shard by shard
	double total[3];
	int rc;
	if ((rc = sum_over_shards(g, 3, total, [&](Shard *s, int, double *v) { return shard_branch_log_likelihood(s, node, length, v, v + 1, v + 2); }))) return rc;
	unpack(total, {{lnl, 1}, {d1, 1}, {d2, 1}});
	return PHYAMD_OK;
}

int phyamd_branch_hessian_diagonal(phyamd_engine *g, int flags, double *lnl, double *d1, double *d2) {
	CHECK_GROUP(g);
	if (!lnl || !d2) return fail(PHYAMD_EINVAL, "null lnl or d2");
	const size_t n = (size_t)1 + 2 * g->N;
	std::vector<double> total(n);
	int rc;
	// per-shard sums added like the gradient's: 2 / 4 / 8 shards cut by the engine's bisection give the one-engine bits
	if ((rc = sum_over_shards(g, n, total.data(), [&](Shard *s, int, double *v) { return shard_branch_hessian_diagonal(s, flags, v); }))) return rc;
	mask_if_not_finite(total[0], total.data() + 1, n - 1);
	unpack(total.data(), {{lnl, 1}, {d1, (size_t)g->N}, {d2, (size_t)g->N}});
	return PHYAMD_OK;
}

// every shard runs the whole batch on its patterns; per-item results are added like phyamd_gradient's
int phyamd_gradient_batch(phyamd_engine *g, int flags, int32_t count, const double *branch_lengths, double *lnl, double *cat_gradient) {
	if (count < 1) return fail(PHYAMD_EINVAL, "phyamd_gradient_batch: count must be >= 1 (got %d)", count);
	if (!branch_lengths || !lnl) return fail(PHYAMD_EINVAL, "phyamd_gradient_batch: null branch_lengths or lnl");
	CHECK_GROUP(g);
	if (group_size(g) == 1) return shard_gradient_batch(g->shards[0], flags, count, branch_lengths, lnl, cat_gradient);
	return sum_batch_over_shards(g, count, lnl, cat_gradient, [&](Shard *s, int, double *l, double *cg) { return shard_gradient_batch(s, flags, count, branch_lengths, l, cg); });
}

// every shard runs the whole batch of trees on its patterns; per-item results are added like phyamd_gradient_batch's
int phyamd_gradient_batch_trees(phyamd_engine *g, int flags, int32_t count, const int32_t *left, const int32_t *right, const int32_t *roots,
                                const double *branch_lengths, double *lnl, double *cat_gradient) {
	if (count < 1) return fail(PHYAMD_EINVAL, "phyamd_gradient_batch_trees: count must be >= 1 (got %d)", count);
	if (!left || !right || !roots || !branch_lengths || !lnl) return fail(PHYAMD_EINVAL, "phyamd_gradient_batch_trees: null left, right, roots, branch_lengths or lnl");
	CHECK_GROUP(g);
	if (group_size(g) == 1) return shard_gradient_batch_trees(g->shards[0], flags, count, left, right, roots, branch_lengths, lnl, cat_gradient);
	return sum_batch_over_shards(g, count, lnl, cat_gradient, [&](Shard *s, int, double *l, double *cg) { return shard_gradient_batch_trees(s, flags, count, left, right, roots, branch_lengths, l, cg); });
}

// every shard runs the whole batch on its own pattern columns of `weights`; per-item results are added like phyamd_gradient_batch's
int phyamd_gradient_batch_weights(phyamd_engine *g, int flags, int32_t count, const double *weights, const double *branch_lengths, double *lnl, double *cat_gradient) {
	static const char *const name = "phyamd_gradient_batch_weights";
	if (count < 1) return fail(PHYAMD_EINVAL, "%s: count must be >= 1 (got %d)", name, count);
	if (!weights || !lnl) return fail(PHYAMD_EINVAL, "%s: null %s", name, !weights ? "weights" : "lnl");
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "%s: null engine", name);
	const size_t P = (size_t)g->P;
	for (size_t b = 0; b < (size_t)count; b++)
		for (size_t k = 0; k < P; k++) {
			const double w = weights[b * P + k];
			if (!(w >= 0.0) || std::isinf(w)) return fail(PHYAMD_EINVAL, "%s: weights of item %zu: pattern %zu has weight %g (a weight is finite and >= 0)", name, b, k, w);
		}
	if (group_size(g) == 1) return shard_gradient_batch_weights(g->shards[0], flags, count, weights, P, branch_lengths, lnl, cat_gradient);
	return sum_batch_over_shards(g, count, lnl, cat_gradient, [&](Shard *s, int i, double *l, double *cg) {
		return shard_gradient_batch_weights(s, flags, count, weights + g->offset[i], P, branch_lengths, l, cg);
	});
}

int phyamd_get_weight_batch_profile(phyamd_engine *g, phyamd_weight_batch_profile *out) {
	// shards choose their paths and chunks themselves: the fewest fast items, the most of everything else; memory adds up
	return merged_profile(g, &Shard::weight_prof, out, [](phyamd_weight_batch_profile &o, const phyamd_weight_batch_profile &p) {
		o.items_fast = std::min(o.items_fast, p.items_fast);
		o.items_sequential = std::max(o.items_sequential, p.items_sequential);
		o.item_chunks = std::max(o.item_chunks, p.item_chunks);
		o.pattern_chunks = std::max(o.pattern_chunks, p.pattern_chunks);
		o.walks = std::max(o.walks, p.walks);
		o.scratch_bytes += p.scratch_bytes;
		o.ms = std::max(o.ms, p.ms);
	});
}

// every shard walks every item on its own patterns: it fills its pattern columns of pattern_lnl and takes its columns of
// replicate_weights; lnl and replicate_lnl are sums over patterns, added in shard order
int phyamd_pattern_log_likelihoods_trees(phyamd_engine *g, int flags, int32_t count, const int32_t *left, const int32_t *right, const int32_t *roots,
                                         const double *branch_lengths, double *lnl, double *pattern_lnl, int32_t replicate_count, const double *replicate_weights,
                                         double *replicate_lnl) {
	static const char *const name = "phyamd_pattern_log_likelihoods_trees";
	if (count < 1) return fail(PHYAMD_EINVAL, "%s: count must be >= 1 (got %d)", name, count);
	if (!branch_lengths || !lnl) return fail(PHYAMD_EINVAL, "%s: null %s", name, !branch_lengths ? "branch_lengths" : "lnl");
	if ((!left || !right || !roots) && (left || right || roots))
		return fail(PHYAMD_EINVAL, "%s: null %s (left, right and roots are given together, or all three are null: the engine's tree)", name,
		            !left ? "left" : !right ? "right" : "roots");
	if (replicate_count < 0) return fail(PHYAMD_EINVAL, "%s: replicate_count must be >= 0 (got %d)", name, replicate_count);
	if (replicate_count > 0 && (!replicate_weights || !replicate_lnl))
		return fail(PHYAMD_EINVAL, "%s: null %s with replicate_count %d", name, !replicate_weights ? "replicate_weights" : "replicate_lnl", replicate_count);
	if (replicate_count == 0 && (replicate_weights || replicate_lnl))
		return fail(PHYAMD_EINVAL, "%s: %s given with replicate_count 0", name, replicate_weights ? "replicate_weights" : "replicate_lnl");
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "%s: null engine", name);
	const size_t P = (size_t)g->P, R = (size_t)replicate_count;
	for (size_t r = 0; r < R; r++)
		for (size_t k = 0; k < P; k++) {
			const double w = replicate_weights[r * P + k];
			if (!(w >= 0.0) || std::isinf(w))
				return fail(PHYAMD_EINVAL, "%s: replicate_weights of replicate %zu: pattern %zu has weight %g (a weight is finite and >= 0)", name, r, k, w);
		}
	if (group_size(g) == 1)
		return shard_pattern_log_likelihoods_trees(g->shards[0], flags, count, left, right, roots, branch_lengths, lnl, pattern_lnl, P, replicate_count, replicate_weights, P,
		                                           replicate_lnl);
	const size_t n = (size_t)count * (1 + R);  // [lnl | replicate_lnl [R][count]]
	std::vector<double> total(n);
	int rc;
	if ((rc = sum_over_shards(g, n, total.data(), [&](Shard *s, int i, double *v) {
		     return shard_pattern_log_likelihoods_trees(s, flags, count, left, right, roots, branch_lengths, v, pattern_lnl ? pattern_lnl + g->offset[i] : nullptr, P,
		                                                replicate_count, R ? replicate_weights + g->offset[i] : nullptr, P, R ? v + count : nullptr);
	     })))
		return rc;
	unpack(total.data(), {{lnl, (size_t)count}, {replicate_lnl, R * count}});
	for (size_t b = 0; b < (size_t)count && R; b++)  // (what a shard masked in band is masked again by the summed lnL)
		if (not_finite(lnl[b]))
			for (size_t r = 0; r < R; r++) replicate_lnl[r * (size_t)count + b] = NAN;
	return PHYAMD_OK;
}

int phyamd_get_site_lnl_profile(phyamd_engine *g, phyamd_site_lnl_profile *out) {
	// the shards choose their chunks themselves: the most of each count; memory adds up
	return merged_profile(g, &Shard::site_prof, out, [](phyamd_site_lnl_profile &o, const phyamd_site_lnl_profile &p) {
		o.chunks = std::max(o.chunks, p.chunks);
		o.replicate_chunks = std::max(o.replicate_chunks, p.replicate_chunks);
		o.lower_slots = std::max(o.lower_slots, p.lower_slots);
		o.scratch_bytes += p.scratch_bytes;
		o.ms = std::max(o.ms, p.ms);
	});
}

int phyamd_get_batch_profile(phyamd_engine *g, phyamd_batch_profile *out) {
	// shards choose their paths themselves: the fewest fast items, the most of everything else
	return merged_profile(g, &Shard::batch_prof, out, [](phyamd_batch_profile &o, const phyamd_batch_profile &p) {
		o.items_fast = std::min(o.items_fast, p.items_fast);
		o.items_sequential = std::max(o.items_sequential, p.items_sequential);
		o.chunks = std::max(o.chunks, p.chunks);
		o.scratch_bytes += p.scratch_bytes;
		o.ms = std::max(o.ms, p.ms);
	});
}

// every shard scores the whole neighbourhood on its patterns; lnl, d1 and d2 are sums over patterns, added in shard order
int phyamd_nni_log_likelihoods(phyamd_engine *g, int flags, const double *central_lengths, double *lnl, double *d1, double *d2) {
	if (!lnl) return fail(PHYAMD_EINVAL, "phyamd_nni_log_likelihoods: null lnl");
	CHECK_GROUP(g);
	const size_t entries = (size_t)3 * g->N, n = 3 * entries;  // [lnl | d1 | d2], each [3][2T-1]
	const bool deriv = d1 || d2;
	std::vector<double> total(n);
	int rc;
	if ((rc = sum_over_shards(g, n, total.data(), [&](Shard *s, int, double *v) { return shard_nni_log_likelihoods(s, flags, central_lengths, deriv, v); }))) return rc;
	nni_mask_derivatives(entries, total.data());
	unpack(total.data(), {{lnl, entries}, {d1, entries}, {d2, entries}});
	return PHYAMD_OK;
}

// the same for 20 states, from the resident partials; one device only, like the other 20-state query calls
int phyamd_nni_log_likelihoods_general(phyamd_engine *g, int flags, const double *central_lengths, double *lnl, double *d1, double *d2) {
	static const char *const name = "phyamd_nni_log_likelihoods_general";
	if (!lnl) return fail(PHYAMD_EINVAL, "%s: null lnl", name);
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "%s: null engine", name);
	if (group_size(g) > 1)
		return fail(PHYAMD_EUNSUPPORTED, "%s: a handle sharded over several devices is out of scope: the call reads one engine's resident partials (use one device)", name);
	const size_t entries = (size_t)3 * g->N;  // [lnl | d1 | d2], each [3][2T-1]
	std::vector<double> out(3 * entries);
	if (int rc = shard_nni_general(g->shards[0], flags, central_lengths, d1 || d2, out.data())) return rc;
	unpack(out.data(), {{lnl, entries}, {d1, entries}, {d2, entries}});
	return PHYAMD_OK;
}

int phyamd_get_nni_profile(phyamd_engine *g, phyamd_nni_profile *out) {
	// the slowest shard is what the caller waits for; memory adds up
	return merged_profile(g, &Shard::nni_prof, out, [](phyamd_nni_profile &o, const phyamd_nni_profile &p) {
		o.scratch_bytes += p.scratch_bytes;
		o.ms = std::max(o.ms, p.ms);
	});
}

// one device only: every iteration of an entry would need its sums across the shards
int phyamd_nni_optimize(phyamd_engine *g, int flags, const double *start_lengths, double lower, double upper, double tolerance, int32_t max_iterations, double *lengths,
                        double *lnl, double *d1, double *d2, int32_t *iterations) {
	static const char *const name = "phyamd_nni_optimize";
	if (!lengths || !lnl) return fail(PHYAMD_EINVAL, "%s: null %s", name, !lengths ? "lengths" : "lnl");
	CHECK_GROUP(g);
	if (!(lower >= 0.0 && lower < upper && std::isfinite(upper))) return fail(PHYAMD_EINVAL, "%s: bounds [%g, %g]: they must be 0 <= lower < upper < inf", name, lower, upper);
	if (!(tolerance > 0.0 && std::isfinite(tolerance))) return fail(PHYAMD_EINVAL, "%s: tolerance %g: it must be finite and positive", name, tolerance);
	if (max_iterations < 1 || max_iterations > 1000) return fail(PHYAMD_EINVAL, "%s: max_iterations %d is outside 1..1000", name, max_iterations);
	if (group_size(g) > 1)
		return fail(PHYAMD_EUNSUPPORTED, "%s: a handle sharded over several devices is out of scope: every iteration of an entry would need a sum across the shards", name);
	return shard_nni_optimize(g->shards[0], flags, NniOptimizeArgs{start_lengths, lower, upper, tolerance, max_iterations, lengths, lnl, d1, d2, iterations});
}

// the same for 20 states, from the resident partials; one device only, like the other 20-state query calls
int phyamd_nni_optimize_general(phyamd_engine *g, int flags, const double *start_lengths, double lower, double upper, double tolerance, int32_t max_iterations, double *lengths,
                                double *lnl, double *d1, double *d2, int32_t *iterations) {
	static const char *const name = "phyamd_nni_optimize_general";
	if (!lengths || !lnl) return fail(PHYAMD_EINVAL, "%s: null %s", name, !lengths ? "lengths" : "lnl");
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "%s: null engine", name);
	if (!(lower >= 0.0 && lower < upper && std::isfinite(upper))) return fail(PHYAMD_EINVAL, "%s: bounds [%g, %g]: they must be 0 <= lower < upper < inf", name, lower, upper);
	if (!(tolerance > 0.0 && std::isfinite(tolerance))) return fail(PHYAMD_EINVAL, "%s: tolerance %g: it must be finite and positive", name, tolerance);
	if (max_iterations < 1 || max_iterations > 1000) return fail(PHYAMD_EINVAL, "%s: max_iterations %d is outside 1..1000", name, max_iterations);
	if (group_size(g) > 1)
		return fail(PHYAMD_EUNSUPPORTED, "%s: a handle sharded over several devices is out of scope: the call reads one engine's resident partials (use one device)", name);
	return shard_nni_optimize_general(g->shards[0], flags, NniOptimizeArgs{start_lengths, lower, upper, tolerance, max_iterations, lengths, lnl, d1, d2, iterations});
}

int phyamd_get_nni_optimize_profile(phyamd_engine *g, phyamd_nni_optimize_profile *out) {
	return merged_profile(g, &Shard::cbopt_prof, out, [](phyamd_nni_optimize_profile &, const phyamd_nni_optimize_profile &) {});  // (never sharded)
}

// one device only: every iteration of a visit would need its sums across the shards
int phyamd_optimize_branch_lengths(phyamd_engine *g, int flags, int32_t count, const int32_t *left, const int32_t *right, const int32_t *roots, const double *branch_lengths,
                                   const uint8_t *optimise, double lower, double upper, double tolerance, int32_t max_iterations, double lnl_tolerance, int32_t max_passes,
                                   double *lengths, double *lnl, double *initial_lnl, int32_t *passes) {
	static const char *const name = "phyamd_optimize_branch_lengths";
	if (!branch_lengths || !lengths || !lnl) return fail(PHYAMD_EINVAL, "%s: null %s", name, !branch_lengths ? "branch_lengths" : !lengths ? "lengths" : "lnl");
	if ((!left || !right || !roots) && (left || right || roots))
		return fail(PHYAMD_EINVAL, "%s: null %s (left, right and roots are given together, or all three are null: the engine's tree)", name,
		            !left ? "left" : !right ? "right" : "roots");
	if (count < 1) return fail(PHYAMD_EINVAL, "%s: count must be >= 1 (got %d)", name, count);
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "%s: null engine", name);
	if (!(lower >= 0.0 && lower < upper && std::isfinite(upper))) return fail(PHYAMD_EINVAL, "%s: bounds [%g, %g]: they must be 0 <= lower < upper < inf", name, lower, upper);
	if (!(tolerance > 0.0 && std::isfinite(tolerance))) return fail(PHYAMD_EINVAL, "%s: tolerance %g: it must be finite and positive", name, tolerance);
	if (max_iterations < 1 || max_iterations > 1000) return fail(PHYAMD_EINVAL, "%s: max_iterations %d is outside 1..1000", name, max_iterations);
	if (!(lnl_tolerance >= 0.0 && std::isfinite(lnl_tolerance))) return fail(PHYAMD_EINVAL, "%s: lnl_tolerance %g: it must be finite and not negative", name, lnl_tolerance);
	if (max_passes < 1 || max_passes > 1000) return fail(PHYAMD_EINVAL, "%s: max_passes %d is outside 1..1000", name, max_passes);
	if (group_size(g) > 1)
		return fail(PHYAMD_EUNSUPPORTED, "%s: a handle sharded over several devices is out of scope: every iteration of a visit would need a sum across the shards", name);
	return shard_branch_optimize(g->shards[0], flags, BranchOptimizeArgs{count, left, right, roots, branch_lengths, optimise, lower, upper, tolerance, max_iterations, lnl_tolerance,
	                                                                      max_passes, lengths, lnl, initial_lnl, passes});
}

int phyamd_get_branch_optimize_profile(phyamd_engine *g, phyamd_branch_optimize_profile *out) {
	return merged_profile(g, &Shard::blopt_prof, out, [](phyamd_branch_optimize_profile &, const phyamd_branch_optimize_profile &) {});  // (never sharded)
}

// every shard scores every row on its patterns; the rows are sums over patterns, added in shard order (NaN cells stay NaN)
int phyamd_spr_log_likelihoods(phyamd_engine *g, int flags, int32_t count, const int32_t *prune, double *lnl) {
	if (count < 1) return fail(PHYAMD_EINVAL, "phyamd_spr_log_likelihoods: count must be >= 1 (got %d)", count);
	if (!lnl) return fail(PHYAMD_EINVAL, "phyamd_spr_log_likelihoods: null lnl");
	CHECK_GROUP(g);
	const WallTime timed{&g->spr_ms};
	return sum_over_shards(g, (size_t)count * g->N, lnl, [&](Shard *s, int, double *v) { return shard_spr_log_likelihoods(s, flags, count, prune, v); });
}

// the same for 20 states, from the resident lowers; one device only, like the other 20-state query calls
int phyamd_spr_log_likelihoods_general(phyamd_engine *g, int flags, int32_t count, const int32_t *prune, double *lnl) {
	static const char *const name = "phyamd_spr_log_likelihoods_general";
	if (!lnl) return fail(PHYAMD_EINVAL, "%s: null lnl", name);
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "%s: null engine", name);
	if (count < 1) return fail(PHYAMD_EINVAL, "%s: count must be >= 1 (got %d)", name, count);
	if (group_size(g) > 1)
		return fail(PHYAMD_EUNSUPPORTED, "%s: a handle sharded over several devices is out of scope: the call reads one engine's resident partials (use one device)", name);
	const WallTime timed{&g->spr_ms};
	return shard_spr_general(g->shards[0], flags, count, prune, lnl);
}

int phyamd_get_spr_profile(phyamd_engine *g, phyamd_spr_profile *out) {
	// candidates and memory add up; the shards choose their chunks themselves: the most
	const int rc = merged_profile(g, &Shard::spr_prof, out, [](phyamd_spr_profile &o, const phyamd_spr_profile &p) {
		o.chunks = std::max(o.chunks, p.chunks);
		o.candidates += p.candidates;
		o.scratch_bytes += p.scratch_bytes;
	});
	if (!rc) out->ms = g->spr_ms;
	return rc;
}

// one device only: every iteration of a visit would need its sums across the shards
int phyamd_spr_optimize(phyamd_engine *g, int flags, int32_t count, const int32_t *prune, double lower, double upper, double tolerance, int32_t max_iterations,
                        double lnl_tolerance, int32_t max_passes, double *lengths, double *lnl, double *initial_lnl, int32_t *passes) {
	static const char *const name = "phyamd_spr_optimize";
	if (count < 1) return fail(PHYAMD_EINVAL, "%s: count must be >= 1 (got %d)", name, count);
	if (!lengths || !lnl) return fail(PHYAMD_EINVAL, "%s: null %s", name, !lengths ? "lengths" : "lnl");
	CHECK_GROUP(g);
	if (!(lower >= 0.0 && lower < upper && std::isfinite(upper))) return fail(PHYAMD_EINVAL, "%s: bounds [%g, %g]: they must be 0 <= lower < upper < inf", name, lower, upper);
	if (!(tolerance > 0.0 && std::isfinite(tolerance))) return fail(PHYAMD_EINVAL, "%s: tolerance %g: it must be finite and positive", name, tolerance);
	if (max_iterations < 1 || max_iterations > 1000) return fail(PHYAMD_EINVAL, "%s: max_iterations %d is outside 1..1000", name, max_iterations);
	if (!(lnl_tolerance >= 0.0 && std::isfinite(lnl_tolerance))) return fail(PHYAMD_EINVAL, "%s: lnl_tolerance %g: it must be finite and not negative", name, lnl_tolerance);
	if (max_passes < 1 || max_passes > 1000) return fail(PHYAMD_EINVAL, "%s: max_passes %d is outside 1..1000", name, max_passes);
	if (group_size(g) > 1)
		return fail(PHYAMD_EUNSUPPORTED, "%s: a handle sharded over several devices is out of scope: every iteration of a visit would need a sum across the shards", name);
	return shard_spr_optimize(g->shards[0], flags,
	                          SprOptimizeArgs{count, prune, lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes, lengths, lnl, initial_lnl, passes});
}

// one device only: the call reads one engine's resident partials
int phyamd_spr_optimize_general(phyamd_engine *g, int flags, int32_t count, const int32_t *prune, double lower, double upper, double tolerance, int32_t max_iterations,
                                double lnl_tolerance, int32_t max_passes, double *lengths, double *lnl, double *initial_lnl, int32_t *passes) {
	static const char *const name = "phyamd_spr_optimize_general";
	if (count < 1) return fail(PHYAMD_EINVAL, "%s: count must be >= 1 (got %d)", name, count);
	if (!lengths || !lnl) return fail(PHYAMD_EINVAL, "%s: null %s", name, !lengths ? "lengths" : "lnl");
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "%s: null engine", name);
	if (!(lower >= 0.0 && lower < upper && std::isfinite(upper))) return fail(PHYAMD_EINVAL, "%s: bounds [%g, %g]: they must be 0 <= lower < upper < inf", name, lower, upper);
	if (!(tolerance > 0.0 && std::isfinite(tolerance))) return fail(PHYAMD_EINVAL, "%s: tolerance %g: it must be finite and positive", name, tolerance);
	if (max_iterations < 1 || max_iterations > 1000) return fail(PHYAMD_EINVAL, "%s: max_iterations %d is outside 1..1000", name, max_iterations);
	if (!(lnl_tolerance >= 0.0 && std::isfinite(lnl_tolerance))) return fail(PHYAMD_EINVAL, "%s: lnl_tolerance %g: it must be finite and not negative", name, lnl_tolerance);
	if (max_passes < 1 || max_passes > 1000) return fail(PHYAMD_EINVAL, "%s: max_passes %d is outside 1..1000", name, max_passes);
	if (group_size(g) > 1)
		return fail(PHYAMD_EUNSUPPORTED, "%s: a handle sharded over several devices is out of scope: the call reads one engine's resident partials (use one device)", name);
	return shard_spr_optimize_general(g->shards[0], flags,
	                                  SprOptimizeArgs{count, prune, lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes, lengths, lnl, initial_lnl, passes});
}

int phyamd_get_spr_optimize_profile(phyamd_engine *g, phyamd_spr_optimize_profile *out) {
	return merged_profile(g, &Shard::tripod_prof, out, [](phyamd_spr_optimize_profile &, const phyamd_spr_optimize_profile &) {});  // (never sharded)
}

// the argument checks of the two distance calls, up to the handle's shards
static int check_pair_distance_arguments(const char *name, phyamd_engine *g, int32_t count, const int32_t *pairs, const double *start, double lower, double upper,
                                         double tolerance, int32_t max_iterations, const double *distances, const double *lnl, const double *d1, const double *d2,
                                         const int32_t *iterations, const double *counts) {
	if (!distances && !counts) return fail(PHYAMD_EINVAL, "%s: null distances and null counts: one of them is the result", name);
	if (!distances && (lnl || d1 || d2 || iterations))
		return fail(PHYAMD_EINVAL, "%s: %s without distances (null distances: the call only counts)", name, lnl ? "lnl" : d1 ? "d1" : d2 ? "d2" : "iterations");
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "%s: null engine", name);
	if (count < 1) return fail(PHYAMD_EINVAL, "%s: count must be >= 1 (got %d)", name, count);
	if (distances) {
		if (!(lower >= 0.0 && lower < upper && std::isfinite(upper))) return fail(PHYAMD_EINVAL, "%s: bounds [%g, %g]: they must be 0 <= lower < upper < inf", name, lower, upper);
		if (!(tolerance > 0.0 && std::isfinite(tolerance))) return fail(PHYAMD_EINVAL, "%s: tolerance %g: it must be finite and positive", name, tolerance);
		if (max_iterations < 1 || max_iterations > 1000) return fail(PHYAMD_EINVAL, "%s: max_iterations %d is outside 1..1000", name, max_iterations);
		for (int32_t p = 0; p < count && start; p++)
			if (!std::isfinite(start[p]) || start[p] < 0.0) return fail(PHYAMD_EINVAL, "%s: start[%d] = %g: a start length is finite and not negative", name, p, start[p]);
	}
	const int64_t T = g->T;
	if (!pairs && (int64_t)count != T * (T - 1) / 2)
		return fail(PHYAMD_EINVAL, "%s: count %d with null pairs: all pairs of %d taxa are %lld", name, count, g->T, (long long)(T * (T - 1) / 2));
	for (int32_t p = 0; p < count && pairs; p++) {
		const int32_t i = pairs[2 * p], j = pairs[2 * p + 1];
		if (i < 0 || i >= g->T || j < 0 || j >= g->T) return fail(PHYAMD_EINVAL, "%s: pairs[%d] = (%d, %d): a taxon index is outside 0..%d", name, p, i, j, g->T - 1);
		if (i == j) return fail(PHYAMD_EINVAL, "%s: pairs[%d] = (%d, %d): a pair is two different taxa", name, p, i, j);
	}
	if (group_size(g) > 1)
		return fail(PHYAMD_EUNSUPPORTED, "%s: a handle sharded over several devices is out of scope: a pair's table would be the sum of the shards' tables", name);
	return PHYAMD_OK;
}

// one device only: a pair's table would be the sum of the shards' tables
int phyamd_pairwise_distances(phyamd_engine *g, int flags, int32_t count, const int32_t *pairs, const double *start, double lower, double upper, double tolerance,
                              int32_t max_iterations, double *distances, double *lnl, double *d1, double *d2, int32_t *iterations, double *counts) {
	if (int rc = check_pair_distance_arguments("phyamd_pairwise_distances", g, count, pairs, start, lower, upper, tolerance, max_iterations, distances, lnl, d1, d2, iterations, counts))
		return rc;
	return shard_pairwise_distances(g->shards[0], flags, PairDistanceArgs{count, pairs, start, lower, upper, tolerance, max_iterations, distances, lnl, d1, d2, iterations, counts, nullptr});
}

int phyamd_pairwise_distances_general(phyamd_engine *g, int flags, int32_t count, const int32_t *pairs, const double *start, double lower, double upper, double tolerance,
                                      int32_t max_iterations, double *distances, double *lnl, double *d1, double *d2, int32_t *iterations, double *counts,
                                      uint64_t *class_members) {
	if (int rc = check_pair_distance_arguments("phyamd_pairwise_distances_general", g, count, pairs, start, lower, upper, tolerance, max_iterations, distances, lnl, d1, d2,
	                                           iterations, counts))
		return rc;
	return shard_pairwise_distances_general(g->shards[0], flags,
	                                        PairDistanceArgs{count, pairs, start, lower, upper, tolerance, max_iterations, distances, lnl, d1, d2, iterations, counts, class_members});
}

int phyamd_get_distance_profile(phyamd_engine *g, phyamd_distance_profile *out) {
	return merged_profile(g, &Shard::dist_prof, out, [](phyamd_distance_profile &, const phyamd_distance_profile &) {});  // (never sharded)
}

// the argument checks of the four placement calls, each written once: an entry point runs them in its own order, the engine's own
// check among them (callers see the first check that fails)

// rows_word: "masks" or "codes", what the caller's rows are called
static int check_placement_score_arguments(const char *name, const char *rows_word, const uint8_t *rows, int32_t queries, int32_t lengths, const double *pendant, double split,
                                    const double *lnl, const int32_t *best_node, const double *best_lnl) {
	if (!lnl && !best_node) return fail(PHYAMD_EINVAL, "%s: null lnl and null best_node: one of them is the result", name);
	if (best_lnl && !best_node) return fail(PHYAMD_EINVAL, "%s: best_lnl without best_node", name);
	if (!rows || !pendant) return fail(PHYAMD_EINVAL, "%s: null %s", name, !rows ? rows_word : "pendant");
	if (queries < 1) return fail(PHYAMD_EINVAL, "%s: queries must be >= 1 (got %d)", name, queries);
	if (lengths < 1) return fail(PHYAMD_EINVAL, "%s: lengths must be >= 1 (got %d)", name, lengths);
	if (!(split >= 0.0 && split <= 1.0)) return fail(PHYAMD_EINVAL, "%s: split %g: it must be in [0, 1]", name, split);
	for (int32_t l = 0; l < lengths; l++)
		if (!std::isfinite(pendant[l]) || !(pendant[l] > 0.0)) return fail(PHYAMD_EINVAL, "%s: pendant[%d] = %g: a pendant length is finite and positive", name, l, pendant[l]);
	return PHYAMD_OK;
}

static int check_placement_optimize_arguments(const char *name, const char *rows_word, const PlacementOptimizeArgs &o) {
	const int32_t *candidates = o.candidates;
	if (!o.masks || !candidates || !o.lengths || !o.lnl)
		return fail(PHYAMD_EINVAL, "%s: null %s", name, !o.masks ? rows_word : !candidates ? "candidates" : !o.lengths ? "lengths" : "lnl");
	if (o.queries < 1) return fail(PHYAMD_EINVAL, "%s: queries must be >= 1 (got %d)", name, o.queries);
	if (o.count < 1) return fail(PHYAMD_EINVAL, "%s: count must be >= 1 (got %d)", name, o.count);
	for (int32_t i = 0; i < o.count; i++)
		if (candidates[2 * (size_t)i] < 0 || candidates[2 * (size_t)i] >= o.queries)
			return fail(PHYAMD_EINVAL, "%s: candidates[%d] = (%d, %d): the query is outside 0..%d", name, i, candidates[2 * (size_t)i], candidates[2 * (size_t)i + 1], o.queries - 1);
	if (o.branches < 1 || o.branches > 7) return fail(PHYAMD_EINVAL, "%s: branches %d is outside 1..7 (bit 0: distal, bit 1: pendant, bit 2: proximal)", name, o.branches);
	if (!(o.split >= 0.0 && o.split <= 1.0)) return fail(PHYAMD_EINVAL, "%s: split %g: it must be in [0, 1]", name, o.split);
	for (int32_t i = 0; i < o.count && o.pendant_start; i++)
		if (!std::isfinite(o.pendant_start[i]) || !(o.pendant_start[i] > 0.0))
			return fail(PHYAMD_EINVAL, "%s: pendant_start[%d] = %g: a pendant length is finite and positive", name, i, o.pendant_start[i]);
	if (!(o.lower >= 0.0 && o.lower < o.upper && std::isfinite(o.upper))) return fail(PHYAMD_EINVAL, "%s: bounds [%g, %g]: they must be 0 <= lower < upper < inf", name, o.lower, o.upper);
	if (!(o.tolerance > 0.0 && std::isfinite(o.tolerance))) return fail(PHYAMD_EINVAL, "%s: tolerance %g: it must be finite and positive", name, o.tolerance);
	if (o.max_iterations < 1 || o.max_iterations > 1000) return fail(PHYAMD_EINVAL, "%s: max_iterations %d is outside 1..1000", name, o.max_iterations);
	if (!(o.lnl_tolerance >= 0.0 && std::isfinite(o.lnl_tolerance))) return fail(PHYAMD_EINVAL, "%s: lnl_tolerance %g: it must be finite and not negative", name, o.lnl_tolerance);
	if (o.max_passes < 1 || o.max_passes > 1000) return fail(PHYAMD_EINVAL, "%s: max_passes %d is outside 1..1000", name, o.max_passes);
	return PHYAMD_OK;
}

// the candidates' nodes, which the engine bounds
static int check_candidate_nodes(const char *name, const phyamd_engine *g, const PlacementOptimizeArgs &o) {
	for (int32_t i = 0; i < o.count; i++)
		if (o.candidates[2 * (size_t)i + 1] < 0 || o.candidates[2 * (size_t)i + 1] >= g->N)
			return fail(PHYAMD_EINVAL, "%s: candidates[%d] = (%d, %d): the node is outside 0..%d", name, i, o.candidates[2 * (size_t)i], o.candidates[2 * (size_t)i + 1], g->N - 1);
	return PHYAMD_OK;
}

// every cell of the queries' rows [queries][P] a state mask (a row is scanned without a branch, and again for the message)
static int check_mask_rows(const char *name, const phyamd_engine *g, int32_t queries, const uint8_t *masks) {
	const size_t P = (size_t)g->P;
	for (int32_t q = 0; q < queries; q++) {
		const uint8_t *row = masks + (size_t)q * P;
		unsigned bad = 0;
		for (size_t k = 0; k < P; k++) bad |= (unsigned)(uint8_t)(row[k] - 1) > 14u;
		if (!bad) continue;
		for (size_t k = 0; k < P; k++)
			if (row[k] < 1 || row[k] > 15)
				return fail(PHYAMD_EINVAL, "%s: masks[%d][%zu] = %d (query %d, pattern %zu): a state mask is 1..15 (bit s: state s; 15: a gap)", name, q, k, (int)row[k], q, k);
	}
	return PHYAMD_OK;
}

// the call's sets, which need no engine ...
static int check_sets(const char *name, int32_t set_count, const uint64_t *sets) {
	if (set_count < 0 || set_count > PLACE_GEN_MAX_SETS) return fail(PHYAMD_EINVAL, "%s: set_count %d is outside 0..%d (a class code is below %d)", name, set_count, PLACE_GEN_MAX_SETS, PLACE_GEN_CLASSES);
	if (set_count > 0 && !sets) return fail(PHYAMD_EINVAL, "%s: null sets with set_count %d", name, set_count);
	for (int32_t q = 0; q < set_count; q++)
		if (sets[q] == 0 || sets[q] >> PLACE_GEN_STATES)
			return fail(PHYAMD_EINVAL, "%s: sets[%d] = 0x%llx: a set has a member and no bit at or above 2^%d (bit s: state s)", name, q, (unsigned long long)sets[q], PLACE_GEN_STATES);
	return PHYAMD_OK;
}

// ... and every cell of the queries' rows [queries][P] a class code over them, which needs its P
static int check_code_rows(const char *name, const phyamd_engine *g, int32_t set_count, int32_t queries, const uint8_t *codes) {
	const size_t P = (size_t)g->P;
	const unsigned top = (unsigned)(PLACE_GEN_STATES + set_count);
	for (int32_t q = 0; q < queries; q++) {
		const uint8_t *row = codes + (size_t)q * P;
		unsigned bad = 0;
		for (size_t k = 0; k < P; k++) bad |= row[k] > top;
		if (!bad) continue;
		for (size_t k = 0; k < P; k++)
			if (row[k] > top)
				return fail(PHYAMD_EINVAL, "%s: codes[%d][%zu] = %d (query %d, pattern %zu): a class code is 0..%u (a state, 20: unknown, 21 + q: sets[q] of the call's %d sets)", name, q, k,
				            (int)row[k], q, k, top, set_count);
	}
	return PHYAMD_OK;
}

static const char *const PLACE_SCORE_ONE_DEVICE = "%s: a handle sharded over several devices is out of scope: a query's best edge would need its sums across the shards";
static const char *const PLACE_OPTIMIZE_ONE_DEVICE = "%s: a handle sharded over several devices is out of scope: every iteration of a visit would need a sum across the shards";

// one device only: a query's lnL on an edge would be the sum of the shards', and its best edge follows from the sums
int phyamd_placement_log_likelihoods(phyamd_engine *g, int flags, int32_t queries, const uint8_t *masks, int32_t lengths, const double *pendant, double split, double *lnl,
                                     int32_t *best_node, double *best_lnl) {
	static const char *const name = "phyamd_placement_log_likelihoods";
	if (int rc = check_placement_score_arguments(name, "masks", masks, queries, lengths, pendant, split, lnl, best_node, best_lnl)) return rc;
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "%s: null engine", name);
	if (int rc = check_mask_rows(name, g, queries, masks)) return rc;
	if (group_size(g) > 1) return fail(PHYAMD_EUNSUPPORTED, PLACE_SCORE_ONE_DEVICE, name);
	return shard_placement(g->shards[0], flags, PlacementArgs{queries, masks, lengths, pendant, split, lnl, best_node, best_lnl});
}

// the same for 20 states: a query cell is a class code over the call's own sets
int phyamd_placement_log_likelihoods_general(phyamd_engine *g, int flags, int32_t queries, const uint8_t *codes, int32_t set_count, const uint64_t *sets, int32_t lengths,
                                             const double *pendant, double split, double *lnl, int32_t *best_node, double *best_lnl) {
	static const char *const name = "phyamd_placement_log_likelihoods_general";
	if (int rc = check_placement_score_arguments(name, "codes", codes, queries, lengths, pendant, split, lnl, best_node, best_lnl)) return rc;
	if (int rc = check_sets(name, set_count, sets)) return rc;
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "%s: null engine", name);
	if (int rc = check_code_rows(name, g, set_count, queries, codes)) return rc;
	if (group_size(g) > 1) return fail(PHYAMD_EUNSUPPORTED, PLACE_SCORE_ONE_DEVICE, name);
	return shard_placement_general(g->shards[0], flags, PlacementGeneralArgs{PlacementArgs{queries, codes, lengths, pendant, split, lnl, best_node, best_lnl}, set_count, sets});
}

int phyamd_get_placement_profile(phyamd_engine *g, phyamd_placement_profile *out) {
	return merged_profile(g, &Shard::place_prof, out, [](phyamd_placement_profile &, const phyamd_placement_profile &) {});  // (never sharded)
}

// one device only: every iteration of a visit would need its sums across the shards
int phyamd_placement_optimize(phyamd_engine *g, int flags, int32_t queries, const uint8_t *masks, int32_t count, const int32_t *candidates, const double *pendant_start,
                              double split, int32_t branches, double lower, double upper, double tolerance, int32_t max_iterations, double lnl_tolerance, int32_t max_passes,
                              double *lengths, double *lnl, double *initial_lnl, int32_t *passes) {
	static const char *const name = "phyamd_placement_optimize";
	const PlacementOptimizeArgs o{queries, masks, count, candidates, pendant_start, split, branches, lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes, lengths, lnl,
	                              initial_lnl, passes};
	if (int rc = check_placement_optimize_arguments(name, "masks", o)) return rc;
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "%s: null engine", name);
	if (int rc = check_candidate_nodes(name, g, o)) return rc;
	if (int rc = check_mask_rows(name, g, queries, masks)) return rc;
	if (group_size(g) > 1) return fail(PHYAMD_EUNSUPPORTED, PLACE_OPTIMIZE_ONE_DEVICE, name);
	return shard_placement_optimize(g->shards[0], flags, o);
}

// the same for 20 states
int phyamd_placement_optimize_general(phyamd_engine *g, int flags, int32_t queries, const uint8_t *codes, int32_t set_count, const uint64_t *sets, int32_t count,
                                      const int32_t *candidates, const double *pendant_start, double split, int32_t branches, double lower, double upper, double tolerance,
                                      int32_t max_iterations, double lnl_tolerance, int32_t max_passes, double *lengths, double *lnl, double *initial_lnl, int32_t *passes) {
	static const char *const name = "phyamd_placement_optimize_general";
	const PlacementOptimizeArgs o{queries, codes, count, candidates, pendant_start, split, branches, lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes, lengths, lnl,
	                              initial_lnl, passes};
	if (int rc = check_placement_optimize_arguments(name, "codes", o)) return rc;
	if (int rc = check_sets(name, set_count, sets)) return rc;
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "%s: null engine", name);
	if (int rc = check_candidate_nodes(name, g, o)) return rc;
	if (int rc = check_code_rows(name, g, set_count, queries, codes)) return rc;
	if (group_size(g) > 1) return fail(PHYAMD_EUNSUPPORTED, PLACE_OPTIMIZE_ONE_DEVICE, name);
	return shard_placement_optimize_general(g->shards[0], flags, PlacementOptimizeGeneralArgs{o, set_count, sets});
}

int phyamd_get_placement_optimize_profile(phyamd_engine *g, phyamd_placement_optimize_profile *out) {
	return merged_profile(g, &Shard::qopt_prof, out, [](phyamd_placement_optimize_profile &, const phyamd_placement_optimize_profile &) {});  // (never sharded)
}

// per-pattern results: every shard fills its own pattern range of the caller's arrays, so a pattern's bits do not depend on the
// shard count.  The NaN rule goes by the handle's lnL (the shards' lnL added like phyamd_log_likelihood's)
int phyamd_state_posteriors(phyamd_engine *g, int flags, int32_t count, const int32_t *nodes, double *posteriors, uint8_t *states) {
	CHECK_GROUP(g);
	ensure_scratch(g, 1);
	int rc;
	if ((rc = for_shards(g, [&](Shard *s, int i) {
		     return shard_state_posteriors(s, flags, count, nodes, (size_t)g->P, posteriors ? posteriors + (size_t)g->offset[i] * g->S : nullptr,
		                                   states ? states + g->offset[i] : nullptr, g->scratch[i].data());
	     })))
		return rc;
	double lnl;
	sum_shards(g, 1, &lnl);
	mask_if_not_finite(lnl, posteriors, (size_t)count * g->P * g->S);
	mask_states_if_not_finite(lnl, states, (size_t)count * g->P);
	return PHYAMD_OK;
}

int phyamd_site_rate_posteriors(phyamd_engine *g, double *posteriors, double *mean_rates) {
	CHECK_GROUP(g);
	if (!posteriors) return fail(PHYAMD_EINVAL, "phyamd_site_rate_posteriors: null posteriors");
	return for_shards(g, [&](Shard *s, int i) {
		return shard_site_rate_posteriors(s, posteriors + (size_t)g->offset[i] * g->C, mean_rates ? mean_rates + g->offset[i] : nullptr);
	});
}

// every shard forms lnl, the gradient and the matrix of its own patterns; they are added over the shards like phyamd_gradient's sums
// (sum_shards: a fixed order of the shard indices).  The NaN rule goes by the handle's lnL
int phyamd_branch_hessian(phyamd_engine *g, int flags, double *lnl, double *gradient, double *hessian) {
	if (!lnl || !hessian) return fail(PHYAMD_EINVAL, "phyamd_branch_hessian: null %s", !lnl ? "lnl" : "hessian");
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "phyamd_branch_hessian: null engine");
	const WallTime timed{&g->bhess_ms};
	if (group_size(g) == 1) return shard_branch_hessian(g->shards[0], flags, lnl, gradient, hessian);
	const size_t N = (size_t)g->N;
	std::vector<double> total(1 + N + N * N);  // [lnl | gradient [N] | hessian [N][N]]
	int rc;
	if ((rc = sum_over_shards(g, total.size(), total.data(), [&](Shard *s, int, double *v) { return shard_branch_hessian(s, flags, v, v + 1, v + 1 + N); }))) return rc;
	mask_if_not_finite(total[0], total.data() + 1, N + N * N);
	unpack(total.data(), {{lnl, 1}, {gradient, N}, {hessian, N * N}});
	return PHYAMD_OK;
}

int phyamd_get_hessian_profile(phyamd_engine *g, phyamd_hessian_profile *out) {
	// memory adds up; the shards choose their chunks themselves: the most
	const int rc = merged_profile(g, &Shard::bhess_prof, out, [](phyamd_hessian_profile &o, const phyamd_hessian_profile &p) {
		o.chunks = std::max(o.chunks, p.chunks);
		o.scratch_bytes += p.scratch_bytes;
	});
	if (!rc) out->ms = g->bhess_ms;
	return rc;
}

int phyamd_get_general_profile(phyamd_engine *g, phyamd_general_profile *out) {
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "phyamd_get_general_profile: null engine");
	if (!out) return fail(PHYAMD_EINVAL, "phyamd_get_general_profile: null out");
	const Shard *s = g->shards[0];  // (the shards choose their tiles themselves, from their own pattern counts: the first one's)
	if (!s->generic) return fail(PHYAMD_EUNSUPPORTED, "phyamd_get_general_profile: %d states (the profile is of the 20 / 60 / 61-state kernels' launches)", s->S);
	*out = s->gen_prof;
	return PHYAMD_OK;
}

int phyamd_get_pass_profile(phyamd_engine *g, phyamd_pass_profile *out) {
	if (!g || g->shards.empty()) return fail(PHYAMD_EINVAL, "phyamd_get_pass_profile: null engine");
	if (!out) return fail(PHYAMD_EINVAL, "phyamd_get_pass_profile: null out");
	const Shard *s = g->shards[0];  // (the shards run the same rule on their own pattern counts and tip data: the first one's)
	if (s->generic) return fail(PHYAMD_EUNSUPPORTED, "phyamd_get_pass_profile: %d states (the profile is of the 4-state kernels' launches)", s->S);
	*out = s->pass_prof;
	return PHYAMD_OK;
}

// device-resident results (one process per GPU: the caller reduces them across processes with ONE RCCL all-reduce)
int phyamd_log_likelihood_device(phyamd_engine *g, double *device_out) {
	CHECK_GROUP(g);
	SINGLE_DEVICE_ONLY(g, "phyamd_log_likelihood_device");
	return shard_log_likelihood_device(g->shards[0], device_out);
}
int phyamd_gradient_device(phyamd_engine *g, int flags, double *device_out) {
	CHECK_GROUP(g);
	SINGLE_DEVICE_ONLY(g, "phyamd_gradient_device");
	return shard_gradient_device(g->shards[0], flags, device_out);
}
int phyamd_parameter_gradient_device(phyamd_engine *g, int flags, double *device_out) {
	CHECK_GROUP(g);
	SINGLE_DEVICE_ONLY(g, "phyamd_parameter_gradient_device");
	return shard_parameter_gradient_device(g->shards[0], flags, device_out);
}

int phyamd_branch_hessian_diagonal_device(phyamd_engine *g, int flags, double *device_out) {
	CHECK_GROUP(g);
	SINGLE_DEVICE_ONLY(g, "phyamd_branch_hessian_diagonal_device");
	return shard_branch_hessian_diagonal_device(g->shards[0], flags, device_out);
}

// --- inspection ---------------------------------------------------------------------------------------------------

int phyamd_get_pattern_log_likelihoods(phyamd_engine *g, double *out) {
	CHECK_GROUP(g);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	return for_shards(g, [&](Shard *s, int i) { return shard_get_pattern_log_likelihoods(s, out + g->offset[i]); });
}

int phyamd_get_partials(phyamd_engine *g, int node, int upper, double *out) {
	CHECK_GROUP(g);
	if (group_size(g) == 1) return shard_get_partials(g->shards[0], node, upper, out);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	// [C][P][S] of the whole pattern list from the shards' [C][P_s][S]
	int rc;
	std::vector<std::vector<double>> part(group_size(g));
	if ((rc = for_shards(g, [&](Shard *s, int i) {
		     part[i].resize((size_t)g->C * s->P * g->S);
		     return shard_get_partials(s, node, upper, part[i].data());
	     })))
		return rc;
	for (int i = 0; i < group_size(g); i++) {
		const size_t ps = (size_t)(g->offset[i + 1] - g->offset[i]);
		for (int c = 0; c < g->C; c++)
			std::memcpy(out + ((size_t)c * g->P + g->offset[i]) * g->S, part[i].data() + (size_t)c * ps * g->S, sizeof(double) * ps * g->S);
	}
	return PHYAMD_OK;
}

int phyamd_get_node_matrices(phyamd_engine *g, int node, int derivative, double *out) {
	CHECK_GROUP(g);
	return shard_get_node_matrices(g->shards[0], node, derivative, out);
}

#include "phyamd_schedule_export.inc"

int phyamd_is_rescaling(phyamd_engine *g) {
	CHECK_GROUP(g);
	int any = 0;  // shards switch on their own lnL (the lazy switch is per shard: the sum does not depend on who rescales)
	for (Shard *s : g->shards) any |= shard_is_rescaling(s);
	return any;
}

int phyamd_get_profile(phyamd_engine *g, phyamd_profile *out) {
	CHECK_GROUP(g);
	if (!out) return fail(PHYAMD_EINVAL, "null out");
	int rc;
	if ((rc = shard_get_profile(g->shards[0], out))) return rc;
	for (int i = 1; i < group_size(g); i++) {  // the slowest shard is what the caller waits for; memory adds up
		phyamd_profile p;
		if ((rc = shard_get_profile(g->shards[i], &p))) return rc;
		out->matrices_ms = std::max(out->matrices_ms, p.matrices_ms);
		out->lower_ms = std::max(out->lower_ms, p.lower_ms);
		out->upper_ms = std::max(out->upper_ms, p.upper_ms);
		out->reduce_ms = std::max(out->reduce_ms, p.reduce_ms);
		out->device_bytes += p.device_bytes;
		out->tiles = std::max(out->tiles, p.tiles);
	}
	return PHYAMD_OK;
}

}  // extern "C"
