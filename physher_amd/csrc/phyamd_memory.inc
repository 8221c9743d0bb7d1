// phyamd_memory.inc -- owning device arrays and the budget a shard allocates them through
// (part of phyamd_engine.hip: one translation unit, internal linkage)

class DeviceBuffer;

// the device memory of one shard: the bytes its arrays hold and the cap on them (cfg.max_device_bytes; <= 0: none) -- or of a
// group of its arrays, whose bytes also count in the shard's budget (`whole`)
struct DeviceBudget {
	explicit DeviceBudget(DeviceBudget *whole = nullptr) : whole(whole) {}
	int64_t cap = 0;
	int64_t bytes = 0;
	DeviceBudget *const whole;
	std::vector<DeviceBuffer *> arrays;  // the arrays bound to this budget
	// on a shard's whole budget: a group of its arrays that is only kept for reuse (the batch scratch).  It never stands in the way:
	// an array outside the group that would not fit -- the cap, or the device itself -- has the group released first
	DeviceBudget *spare = nullptr;
	void release_all();
};

// device memory owned by one array, bound to a budget for its lifetime (none: a scoped temporary, not counted).  Allocating checks
// the cap and adds the bytes; release() and the destructor free the array and take exactly those bytes off again.
class DeviceBuffer {
public:
	explicit DeviceBuffer(DeviceBudget *budget) : budget_(budget) {
		if (budget_) budget_->arrays.push_back(this);
	}
	DeviceBuffer(const DeviceBuffer &) = delete;
	DeviceBuffer &operator=(const DeviceBuffer &) = delete;
	~DeviceBuffer() {
		release();
		if (budget_) budget_->arrays.erase(std::find(budget_->arrays.begin(), budget_->arrays.end(), this));
	}
	size_t bytes() const { return bytes_; }
	void release() {
		if (!p_) return;
		(void)hipFree(p_);
		for (DeviceBudget *b = budget_; b; b = b->whole) b->bytes -= (int64_t)bytes_;
		p_ = nullptr;
		bytes_ = 0;
	}
	void swap(DeviceBuffer &o) {  // (two arrays of one budget)
		std::swap(p_, o.p_);
		std::swap(bytes_, o.bytes_);
	}
	// at least `bytes` (0: one), whatever the element type; see reserve
	int ensure_bytes(size_t bytes) { return reserve(std::max<size_t>(bytes, 1), nullptr); }

protected:
	// at least `bytes`: kept if it holds as many, else freed and allocated anew (*grew: the old contents are gone)
	int reserve(size_t bytes, bool *grew) {
		if (grew) *grew = false;
		if (p_ && bytes_ >= bytes) return PHYAMD_OK;
		release();
		DeviceBudget *spare = nullptr;  // the spare group, if this array is not of it and it holds anything
		for (DeviceBudget *b = budget_; b; b = b->whole)
			if (b->spare && b->spare != budget_ && b->spare->bytes > 0) spare = b->spare;
		for (DeviceBudget *b = budget_; b; b = b->whole) {
			if (b->cap > 0 && b->bytes + (int64_t)bytes > b->cap && spare) {
				spare->release_all();
				spare = nullptr;
			}
			if (b->cap > 0 && b->bytes + (int64_t)bytes > b->cap)
				return fail(PHYAMD_ENOMEM, "max_device_bytes (%lld) would be exceeded: %lld bytes resident, %zu more requested", (long long)b->cap,
				            (long long)b->bytes, bytes);
		}
		void *p = nullptr;
		if (spare && hipMalloc(&p, bytes) != hipSuccess) {  // (the device is full of spare arrays)
			(void)hipGetLastError();
			p = nullptr;
			spare->release_all();
		}
		if (!p) HIP_TRY(hipMalloc(&p, bytes));
		p_ = p;
		bytes_ = bytes;
		for (DeviceBudget *b = budget_; b; b = b->whole) b->bytes += (int64_t)bytes;
		if (grew) *grew = true;
		return PHYAMD_OK;
	}
	void *p_ = nullptr;
	size_t bytes_ = 0;

private:
	DeviceBudget *const budget_;
};

void DeviceBudget::release_all() {
	for (DeviceBuffer *a : arrays) a->release();
}

template <typename T>
class DeviceArray : public DeviceBuffer {
public:
	explicit DeviceArray(DeviceBudget *budget = nullptr) : DeviceBuffer(budget) {}
	operator T *() const { return static_cast<T *>(p_); }
	T *get() const { return static_cast<T *>(p_); }
	size_t size() const { return bytes_ / sizeof(T); }
	// at least `count` elements (0: one); see reserve
	int ensure(size_t count, bool *grew = nullptr) { return reserve(std::max<size_t>(count, 1) * sizeof(T), grew); }
};

// What a call needs of a group of scratch arrays to work on n items at once: array by array, so many bytes per item and so many
// whatever n.  The one description of a call's scratch: the bytes a chunk is sized by, whether what is held serves n items, and
// the allocation itself are all read off this list.
struct ScratchPlan {
	struct Entry {
		DeviceBuffer *array;
		size_t item_bytes, fixed_bytes;
		bool once;  // item_bytes are counted for every item but allocated once (spr_plan)
		size_t bytes(size_t n) const { return fixed_bytes + (once ? 1 : n) * item_bytes; }
	};
	std::vector<Entry> entries;
	void add(DeviceBuffer &array, size_t item_bytes, size_t fixed_bytes = 0, bool once = false) { entries.push_back(Entry{&array, item_bytes, fixed_bytes, once}); }
	size_t item_bytes() const {
		size_t b = 0;
		for (const Entry &x : entries) b += x.item_bytes;
		return b;
	}
	size_t fixed_bytes() const {
		size_t b = 0;
		for (const Entry &x : entries) b += x.fixed_bytes;
		return b;
	}
	// items that fit in `room` bytes (a double: compared before it is cut to a count; below 1: not even one)
	double items_in(double room) const { return std::floor((room - (double)fixed_bytes()) / (double)item_bytes()); }
	// the arrays hold n items already
	bool held(size_t n) const {
		return std::all_of(entries.begin(), entries.end(), [n](const Entry &x) { return x.array->bytes() >= x.bytes(n); });
	}
	// every array at least at its size for n items (an array that holds as much is kept: DeviceBuffer::reserve)
	int allocate(size_t n) const {
		for (const Entry &x : entries)
			if (int rc = x.array->ensure_bytes(x.bytes(n))) return rc;
		return PHYAMD_OK;
	}
	// also what `other` needs: its entries this plan lacks, and of an array both name the larger sizes
	void merge(const ScratchPlan &other) {
		for (const Entry &o : other.entries) {
			const auto mine = std::find_if(entries.begin(), entries.end(), [&o](const Entry &x) { return x.array == o.array; });
			if (mine == entries.end()) entries.push_back(o);
			else mine->item_bytes = std::max(mine->item_bytes, o.item_bytes), mine->fixed_bytes = std::max(mine->fixed_bytes, o.fixed_bytes);
		}
	}
};
