// phyamd_patterns.inc -- site-pattern compression on the device (SURVEY 8f.3), bit-exact with new_SitePattern
// (sitepattern.c:186-251) including the ORDER of the patterns, which in the reference is the iteration order of its
// chained hash table (hashtable.c).  Included by phyamd_engine.hip inside its anonymous namespace.
//
// The reference inserts the columns one by one; what comes out depends only on
//   * which columns are equal                          -> groups, their sizes (weights) and first sites,
//   * the order in which distinct columns first appear -> insertion rank r of a group,
//   * the table's growth history (193 buckets, next prime when a NEW key arrives at length == ceil(0.65 size); growth
//     re-links every chain head-first walking the old buckets in order; new keys go to the head of their chain),
// so the O(T L) part (hashing, grouping) is done with one pass over the alignment and radix sorts, and the order is
// rebuilt from (hash, rank) per group.  Chain order, for two keys of one bucket of table j at the end of epoch j
// (epoch(x) = the table x was first inserted into):
//     both inserted in epoch j:   the later one is nearer the head;
//     one inserted, one carried:  the inserted one is nearer the head;
//     both carried from table j-1: the one from the higher old bucket is nearer the head; within one old bucket the
//                                  old order is reversed.
// This is a lexicographic comparison of per-level components with alternating direction, i.e. a sequence of stable
// sorts from the oldest table to the newest, then by final bucket.
//
// Equal 64-bit sort keys (the reference's 32-bit hash + an independent 32-bit hash) are verified column against column;
// a genuine collision between different columns is reported as PHYAMD_EUNSUPPORTED ("use the host path"), never folded.

// growth sequence of the reference's table (hashtable.c:61-70)
constexpr unsigned PATTERN_PRIMES[] = {5,        53,       97,        193,       389,       769,       1543,      3079,      6151,
                                       12289,    24593,    49157,     98317,     196613,    393241,    786433,    1572869,   3145739,
                                       6291469,  12582917, 25165843,  50331653,  100663319, 201326611, 402653189, 805306457, 1610612741};
constexpr int PATTERN_PRIME_COUNT = sizeof(PATTERN_PRIMES) / sizeof(PATTERN_PRIMES[0]);
constexpr int PATTERN_FIRST_PRIME = 3;  // 193 buckets: first prime >= 100 (sitepattern.c:200)

struct PatternEpochs {
	unsigned size[PATTERN_PRIME_COUNT];
	unsigned limit[PATTERN_PRIME_COUNT];  // a new key arriving at this length grows the table first
	int last;                            // index of the final table
};

// one thread per site: optional symbol -> code translation (in place), the reference's key hash (sitepattern.c:71-79 +
// the mixer of hashtable.c:188-197) and an independent FNV-1a hash; codes: [T][L]
__global__ __launch_bounds__(256) void k_pattern_hash(int T, size_t L, uint8_t *__restrict__ codes, const uint8_t *__restrict__ lut,
                                                     unsigned long long *__restrict__ keys, unsigned *__restrict__ sites) {
	const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (s >= L) return;
	unsigned h = 0, g = 2166136261u;
	for (int t = 0; t < T; t++) {
		unsigned v = codes[(size_t)t * L + s];
		if (lut) {
			v = lut[v];
			codes[(size_t)t * L + s] = (uint8_t)v;
		}
		h = t == 0 ? v : h ^ (v + 0x9e3779b9u + (h << 6) + (h >> 2));
		g = (g ^ v) * 16777619u;
	}
	h += ~(h << 9);
	h ^= (h >> 14) | (h << 18);
	h += h << 4;
	h ^= (h >> 10) | (h << 22);
	keys[s] = ((unsigned long long)h << 32) | g;
	sites[s] = (unsigned)s;
}

// sorted position i: head of a group?  Equal keys are checked column against column (neighbours suffice: equality is transitive)
__global__ __launch_bounds__(256) void k_pattern_heads(int T, size_t L, const uint8_t *__restrict__ codes, const unsigned long long *__restrict__ keys,
                                                      const unsigned *__restrict__ sites, unsigned *__restrict__ head, int *__restrict__ collision) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= L) return;
	const bool is_head = i == 0 || keys[i] != keys[i - 1];
	head[i] = is_head ? 1u : 0u;
	if (is_head) return;
	const size_t a = sites[i], b = sites[i - 1];
	bool same = true;
	for (int t = 0; t < T; t++) same &= codes[(size_t)t * L + a] == codes[(size_t)t * L + b];
	if (!same) atomicOr(collision, 1);
}

// gid = inclusive scan of head - 1.  Per group: first sorted position (stable sort: its site is the first occurrence)
__global__ __launch_bounds__(256) void k_pattern_groups(size_t L, const unsigned *__restrict__ head, const unsigned *__restrict__ scan,
                                                       const unsigned long long *__restrict__ keys, const unsigned *__restrict__ sites,
                                                       unsigned *__restrict__ gstart, unsigned *__restrict__ gsite, unsigned *__restrict__ ghash,
                                                       unsigned *__restrict__ gid) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= L || !head[i]) return;
	const unsigned g = scan[i] - 1;
	gstart[g] = (unsigned)i;
	gsite[g] = sites[i];
	ghash[g] = (unsigned)(keys[i] >> 32);
	gid[g] = g;
}

__global__ __launch_bounds__(256) void k_pattern_ranks(unsigned n, const unsigned *__restrict__ order, unsigned *__restrict__ rank) {
	const unsigned i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) rank[order[i]] = i;
}

// sort component of level `level` for every group in its current position (see the header comment)
__global__ __launch_bounds__(256) void k_pattern_component(unsigned n, int level, PatternEpochs ep, const unsigned *__restrict__ perm,
                                                          const unsigned *__restrict__ rank, const unsigned *__restrict__ ghash,
                                                          unsigned long long *__restrict__ key) {
	const unsigned i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const unsigned g = perm[i], r = rank[g];
	int e = PATTERN_FIRST_PRIME;
	while (r >= ep.limit[e]) e++;
	const bool forward = ((ep.last - level) & 1) == 0;
	unsigned long long k = 0;
	if (level == e) k = forward ? (unsigned long long)(0xFFFFFFFFu - r) : ((1ull << 32) | r);
	else if (level > e) {
		const unsigned b = ghash[g] % ep.size[level - 1];
		k = forward ? ((1ull << 32) | (0xFFFFFFFFu - b)) : (unsigned long long)b;
	}
	key[i] = k;
}

__global__ __launch_bounds__(256) void k_pattern_bucket(unsigned n, unsigned size, const unsigned *__restrict__ perm, const unsigned *__restrict__ ghash,
                                                       unsigned long long *__restrict__ key) {
	const unsigned i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) key[i] = ghash[perm[i]] % size;
}

// patterns[t][k] = codes[t][first site of the k-th group]; weights[k] = group size
__global__ __launch_bounds__(256) void k_pattern_emit(int T, size_t L, unsigned n, const uint8_t *__restrict__ codes, const unsigned *__restrict__ perm,
                                                     const unsigned *__restrict__ gstart, const unsigned *__restrict__ gsite,
                                                     uint8_t *__restrict__ patterns, double *__restrict__ weights) {
	const unsigned k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n) return;
	const unsigned g = perm[k];
	if (blockIdx.y == 0) weights[k] = (double)((g + 1 < n ? gstart[g + 1] : (unsigned)L) - gstart[g]);
	const size_t site = gsite[g];
	for (int t = blockIdx.y; t < T; t += gridDim.y) patterns[(size_t)t * n + k] = codes[(size_t)t * L + site];
}

int compress_patterns_device(int device, int T, int64_t L64, const uint8_t *const *rows, const uint8_t *lut, int32_t *pattern_count, uint8_t *patterns,
                             double *weights) {
	if (T < 1 || L64 < 1 || !rows || !pattern_count || !patterns || !weights) return fail(PHYAMD_EINVAL, "bad argument");
	if (L64 > 0x7FFFFFFF) return fail(PHYAMD_EUNSUPPORTED, "more than 2^31 - 1 sites");
	int ndev = 0;
	HIP_TRY(hipGetDeviceCount(&ndev));
	if (ndev == 0) return fail(PHYAMD_EDEVICE, "no HIP device visible");
	if (device >= ndev) return fail(PHYAMD_EINVAL, "device %d out of range (%d visible)", device, ndev);
	if (device >= 0) HIP_TRY(hipSetDevice(device));
	const size_t L = (size_t)L64;
	hipStream_t st = nullptr;  // the null stream: this is a one-off, synchronous call
	// scoped temporaries, not counted against any engine's memory
	DeviceArray<uint8_t> codes, lutd, outp;
	DeviceArray<unsigned long long> keys0, keys1;
	DeviceArray<unsigned> val0, val1, head, scan, gstart, gsite, ghash, rank;
	DeviceArray<int> flag;
	DeviceArray<char> tmp;
	DeviceArray<double> outw;
	int rc;
	if ((rc = codes.ensure((size_t)T * L)) || (rc = keys0.ensure(L)) || (rc = keys1.ensure(L)) || (rc = val0.ensure(L)) || (rc = val1.ensure(L)) ||
	    (rc = head.ensure(L)) || (rc = scan.ensure(L)) || (rc = flag.ensure(1)))
		return rc;
	HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), st));
	for (int t = 0; t < T; t++) {
		if (!rows[t]) return fail(PHYAMD_EINVAL, "row %d is null", t);
		HIP_TRY(hipMemcpyAsync(codes + (size_t)t * L, rows[t], L, hipMemcpyHostToDevice, st));
	}
	if (lut) {
		if ((rc = lutd.ensure(256))) return rc;
		HIP_TRY(hipMemcpyAsync(lutd, lut, 256, hipMemcpyHostToDevice, st));
	}
	const unsigned lb = (unsigned)((L + 255) / 256);
	hipLaunchKernelGGL(k_pattern_hash, dim3(lb), dim3(256), 0, st, T, L, codes, lutd, keys0, val0);
	// one temporary block serves every sort / scan below (sizes queried for the largest problem)
	size_t b1 = 0, b2 = 0, b3 = 0;
	HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b1, keys0.get(), keys1.get(), val0.get(), val1.get(), (int)L, 0, 64, st));
	HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, b2, head.get(), scan.get(), (int)L, st));
	HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, b3, val0.get(), val1.get(), val0.get(), val1.get(), (int)L, 0, 32, st));
	size_t tmp_bytes = std::max(b1, std::max(b2, b3));
	if ((rc = tmp.ensure(tmp_bytes))) return rc;
	HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys0.get(), keys1.get(), val0.get(), val1.get(), (int)L, 0, 64, st));
	const unsigned long long *skeys = keys1;
	const unsigned *ssites = val1;
	hipLaunchKernelGGL(k_pattern_heads, dim3(lb), dim3(256), 0, st, T, L, codes, skeys, ssites, head, flag);
	tmp_bytes = std::max(b1, std::max(b2, b3));
	HIP_TRY(hipcub::DeviceScan::InclusiveSum(tmp, tmp_bytes, head.get(), scan.get(), (int)L, st));
	unsigned n = 0;
	int collided = 0;
	HIP_TRY(hipMemcpyAsync(&n, scan + (L - 1), sizeof(unsigned), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&collided, flag, sizeof(int), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (collided) return fail(PHYAMD_EUNSUPPORTED, "two different columns share both hashes: compress this alignment on the host");
	if ((rc = gstart.ensure(n)) || (rc = gsite.ensure(n)) || (rc = ghash.ensure(n)) || (rc = rank.ensure(n))) return rc;
	// group tables; val0 / keys0 are free again: val0 = group ids, then the working permutation
	hipLaunchKernelGGL(k_pattern_groups, dim3(lb), dim3(256), 0, st, L, head, scan, skeys, ssites, gstart, gsite, ghash, val0);
	const unsigned nb = (n + 255) / 256;
	// insertion rank = position among the groups ordered by first site (head/scan are free: reuse as sort buffers)
	unsigned *site_sorted = head, *order = scan;
	tmp_bytes = std::max(b1, std::max(b2, b3));
	HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, gsite.get(), site_sorted, val0.get(), order, (int)n, 0, 32, st));
	hipLaunchKernelGGL(k_pattern_ranks, dim3(nb), dim3(256), 0, st, n, order, rank);
	PatternEpochs ep;
	for (int j = 0; j < PATTERN_PRIME_COUNT; j++) {
		ep.size[j] = PATTERN_PRIMES[j];
		ep.limit[j] = (unsigned)std::ceil(PATTERN_PRIMES[j] * 0.65);
	}
	ep.limit[PATTERN_PRIME_COUNT - 1] = 0xFFFFFFFFu;
	ep.last = PATTERN_FIRST_PRIME;
	while (n - 1 >= ep.limit[ep.last]) ep.last++;
	// stable sorts, oldest table first; perm ping-pongs between val0 and val1, keys between keys0 and keys1
	unsigned *perm = val0, *perm_alt = val1;
	unsigned long long *key = keys0, *key_alt = keys1;
	for (int level = PATTERN_FIRST_PRIME; level <= ep.last + 1; level++) {
		const bool final_pass = level == ep.last + 1;
		if (final_pass) hipLaunchKernelGGL(k_pattern_bucket, dim3(nb), dim3(256), 0, st, n, ep.size[ep.last], perm, ghash, key);
		else hipLaunchKernelGGL(k_pattern_component, dim3(nb), dim3(256), 0, st, n, level, ep, perm, rank, ghash, key);
		tmp_bytes = std::max(b1, std::max(b2, b3));
		HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, key, key_alt, perm, perm_alt, (int)n, 0, final_pass ? 32 : 33, st));
		std::swap(perm, perm_alt);
	}
	if ((rc = outp.ensure((size_t)T * n)) || (rc = outw.ensure(n))) return rc;
	hipLaunchKernelGGL(k_pattern_emit, dim3(nb, (unsigned)std::min(T, 64)), dim3(256), 0, st, T, L, n, codes, perm, gstart, gsite, outp, outw);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(patterns, outp, (size_t)T * n, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(weights, outw, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	*pattern_count = (int32_t)n;
	return PHYAMD_OK;
}
