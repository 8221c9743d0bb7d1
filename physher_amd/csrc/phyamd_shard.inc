// phyamd_shard.inc -- state of one engine on one GPU (one pattern shard) and the form of its stored 4-state lowers
// (part of phyamd_engine.hip: one translation unit, internal linkage)

// what a stored 4-state lower array holds: the reference's p_n (with its rescaling), or -- read by the two streamed walks only --
// t_n = P_n p_n (their TF), unscaled or rescaled by powers of two per category (SCALE == 2)
enum class LowerForm { Reference, Carried, CarriedExp2 };

// schedule counts the pattern tiles are sized by (tile_working_set)
struct ScheduleCounts { int core_count, upper_slots, widest; };

struct Shard {
	phyamd_config cfg{};
	// device memory: every owning d_* array below is allocated through one of these budgets (phyamd_memory.inc)
	DeviceBudget mem;             // all of it, capped by cfg.max_device_bytes (the profile's device_bytes)
	DeviceBudget tile_mem{&mem};  // the arrays sized by the pattern tile, which a re-tile drops (free_pattern_storage)
	int T = 0, N = 0, P = 0, S = 0, C = 0, root = -1;
	int G = 1;  // pattern groups (waves along z) per workgroup
	bool generic = false;  // S != 4: MFMA kernels, plane layout [C][S][Pp]
	int Pp = 0;            // padded plane stride (generic)
	int nblk_root = 0;     // workgroups of k_root_finish (generic)
	int nblk_lower = 0;    // pattern blocks of the post-order kernels
	int nblk_walk = 0, nblk_walk_upper = 0;  // pattern blocks of the tree-walk kernels
	int lower_walk_slots[2] = {0, 0};  // resident workgroups of k_lower4_walk at one / two patterns per thread
	int gen_slots[3][2] = {};          // resident workgroups of the 20 / 60 / 61-state kernels on this engine's device: [lower, upper, upper FOLD][SCALE]
	int lnl_blocks = 0;    // entries of d_lnl_part the last post-order pass wrote
	int grad_blocks = 0;   // entries per row of d_gpart the last pre-order pass wrote
	size_t gpart_row = 0;  // allocated entries per row
	// which products of the inputs are current: written only by "what each input invalidates" below
	struct State {
		// stored lowers, with incremental (dirty-node) post-order updates: D1, treelikelihood.c:73-114, 1645-1734
		bool all_dirty = true;         // they are not those of the current inputs: recompute every node
		std::vector<int> changed;      // ... they are, except above these nodes, whose branch length changed since the last evaluation
		bool force_root = false;       // ... except for the root's outputs (lnL_k, w_k / L_k, lnL), which belong to a discarded state
		bool upper_valid = false;      // d_upper holds the uppers of a gradient at the current inputs (resident: of a keep-partials one)
		int path_node = -1;            // node whose upper d_path_upper holds (-1: none)
		bool matrices_dirty = true;    // P(t) with the tip tables / MFMA images
		bool qimg_dirty = true;        // 20 / 60 / 61 states: the images of Q and diag(pi) Q
		bool qpi_dirty = true;         // 4 states: diag(pi) Q
		int qp_kind = -1;              // which Qf the images of Qf P(t) hold: 0 = Q (pi folded into the uppers), 1 = diag(pi) Q, -1 = none
		bool params_dirty = true;      // U^-1 dQ U
		bool stored_valid = false;     // the MCMC stored state below
		bool tiled_eval_done = false;  // d_total holds the sums of a tiled evaluation at the current inputs
		bool tiled_root_term = false;  // ... and d_result the summed root frequency term of a tiled parameter gradient
		unsigned long tip_epoch = 1;   // the tip data in d_tipmask (the mask words: as of mstream_epoch)
		bool spr_lists_dirty = true;   // spr_ops and spr_tin / spr_tout are not the current tree's
	} state;
	bool incremental_pass = false;
	std::vector<NodeOp> inc_ops;      // ops of the dirty core nodes, by level
	std::vector<int> inc_level_off;
	DeviceArray<NodeOp> d_inc_ops{&mem};
	const std::vector<int> *act_level_off = nullptr;
	NodeOp *act_lower_ops = nullptr;
	bool level_upper_needed = false;  // a Levels pre-order pass has run: d_upper holds the level schedule's slots (ensure_upper_storage)
	// MCMC store / restore (_singleTreeLikelihood_store, _treelikelihood_handle_restore: treelikelihood.c:116-161): after a
	// store every stored node has two slots (slot = core index, + core_count for the second); an evaluation never writes the
	// slot the stored state lives in, so restore is an index flip (plus re-integrating the root), not a recomputation
	struct Stored {
		std::vector<double> lengths, model, freqs, rates, props;
		std::vector<int32_t> core_index;  // node -> slot of the stored state
		bool have_eigen = false, scaling_on = false;
		unsigned long epoch = 0;
		double lnl = 0.0;
	} stored;
	// pattern tiling (cfg.max_device_bytes): P = patterns per tile (what every kernel sees), Ptot = the caller's count;
	// tip data, weights and per-pattern lnL of all tiles stay resident, the partial arrays are reused tile after tile
	int Ptot = 0, tiles = 1;
	DeviceArray<uint8_t> d_tip_all{&tile_mem};  // [T][Ptot]
	DeviceArray<double> d_weights_all{&tile_mem}, d_plk_all{&tile_mem}, d_total{&tile_mem};
	unsigned long schedule_epoch = 0;  // bumped whenever slots are reassigned from scratch
	bool two_slots = false;            // d_lower / d_lscale hold 2 * core_count slots
	bool generic_fusion = true;  // 20 states: cherries fused into their parents' ops (PHYAMD_GEN_FUSION = 0: every node stored)
	bool walk_enabled = true;  // PHYAMD_WALK = 0: no walk lists, every pass runs the level kernels
	DeviceArray<int> d_gen_walk_counter{&mem};  // work-unit counter of the walk
	int gen_walk_slots[1] = {0};  // resident workgroups of k_lower_gen_walk
	DeviceArray<NodeOp> d_walk_lower_ops{&mem}, d_walk_upper_ops{&mem};
	DeviceArray<NodeOp> d_walk_lower_chunk_ops{&mem};
	DeviceArray<int> d_walk_lower_chunk_off{&mem};
	DeviceArray<NodeOp> d_walk_chunk_ops{&mem};
	DeviceArray<int> d_walk_chunk_off{&mem};
	// streamed pre-order walk (phyamd_walk4s.inc): flattened ops of the chunked list, mask words in walk order, walk-order slab
	bool upper_stream_capped = false;    // the cap left no room for the pre-order walk's mask words / table blocks: neither walk streams
	bool lower_stream_capped = false;    // ... for the post-order walk's (or its root terms): the post-order walk does not stream
	int xcd_map = 1;                    // PHYAMD_XCD_MAP = 0: streamed walks with consecutive workgroup ids per block group (A/B; see xcd_position)
	DeviceArray<LowerDesc> d_lstream_ops{&mem};
	DeviceArray<LowerChunk> d_lstream_chunks{&mem};
	DeviceArray<int> d_stream_op_tips{&mem}, d_stream_flag{&mem}, d_stream_op_deep{&mem}, d_stream_pair_tab{&mem};
	DeviceArray<char> d_optab{&mem};     // [C][ops] table blocks of OPBLK_BYTES, rebuilt from the matrices every evaluation
	bool stream_ambiguous = false;       // the tip data hold partial ambiguity codes: the AMBIG instantiation of the streamed walk
	bool stream_unsupported = false;     // the tip data the mask words were built for hold an empty state mask: the table-gather walks
	DeviceArray<StreamDesc> d_stream_ops{&mem};
	DeviceArray<StreamChunk> d_stream_chunks{&mem};
	DeviceArray<int> d_stream_row_entries{&mem}, d_stream_site_tab{&mem}, d_stream_qnode{&mem}, d_oct_lo{&mem};
	DeviceArray<uint32_t> d_mstream{&tile_mem};
	size_t mstride = 0;
	unsigned long mstream_epoch = 0;     // state.tip_epoch of the tip data the mask words were built from
	std::vector<int> mstream_layout;     // stream_tab.row_entries the device stream was built for
	double *d_gslab = nullptr;           // the walk-order slab, in d_gpart's storage
	DeviceArray<double> d_oct{&mem};
	bool slab_walk_order = false;        // the last pre-order pass wrote d_gslab (walk order), not d_gpart
	// sums over pattern blocks (reduce_block_sums): bisection levels of this engine's block range (3 = eight segments; a shard that
	// holds 1 / 2^k of a larger range cut by the same bisection runs with 3 - k), and what the segment table on the device is for
	int reduce_levels = 3, seg_nb[2] = {-1, -1}, seg_levels[2] = {-1, -1};
	bool lnl_per_block = false;          // d_lnl_part holds one entry per block of 64 patterns (the tree walk)
	DeviceArray<double> d_Lc{&tile_mem};  // [C][P] per-category site likelihoods at the root
	DeviceArray<double> d_imgs{&mem};  // generic: MFMA fragment images of P(t) per (node, category), then of Q (k_matrix_images)
	DeviceArray<double> d_qp_mats{&mem};  // generic: Qf P(t) per (tip, category), row-major, and its fragment images (k_tip_rate_products): the
	DeviceArray<double> d_qp_imgs{&mem};  // branch term of a tip child is a column of that product, looked up instead of multiplied out
	DeviceArray<double> d_inv_part{&tile_mem};  // partial sums of k_root_invariant_term
	int device = 0;
	hipStream_t stream = nullptr;
	bool own_stream = false;

	std::vector<int32_t> left, right;
	std::vector<double> lengths, model, freqs, rates, props;
	// lengths: what the device holds (the root's entry 0).  lengths_sent: the caller's own values by node id, the entry at the
	// root's id too: a new topology with another root takes the old root's branch from here (shard_set_topology)
	std::vector<double> lengths_sent;
	std::vector<uint8_t> explicit_host;
	bool have_topology = false, have_lengths = false, have_eigen = false, have_freqs = false, have_rates = false, have_weights = false;
	std::vector<uint8_t> tip_set;
	bool scaling_on = false;
	// the form of the stored 4-state lowers in the slots core_index points at now, and the policy that decides it (below,
	// "what d_lower holds"): reference_form_only = some reader has needed the reference's form, every later post-order pass writes it
	LowerForm lower_form = LowerForm::Reference;
	bool reference_form_only = false;
	bool exp2_on = true, tform_on = true;  // PHYAMD_SCALE_EXP2 = 0 / PHYAMD_STREAM_TFORM = 0: the streamed walks never write CarriedExp2 / Carried
	bool lower_park2_on = true;            // PHYAMD_LOWER_PARK2 = 0: the post-order schedule parks in one slot only (ScheduleOptions)
	bool stream_pairs_on = true;           // PHYAMD_STREAM_PAIRS = 0: the plain pre-order pass runs every DEEP child's op on its own (stream_pairs, phyamd_tree_schedule.h)
	bool stream_elide_on = true;           // PHYAMD_STREAM_ELIDE = 0: the streamed walks store every stored node (stream_elide, phyamd_tree_schedule.h)
	bool stream_keep_on = true;            // PHYAMD_STREAM_KEEP = 0: an elided node's op always requests its stored child's plane again (stream_keep, phyamd_tree_schedule.h)
	DeviceArray<int> d_lexp{&tile_mem}, d_uexp{&tile_mem}, d_Ec{&tile_mem}, d_Eroot{&tile_mem};  // exponents: [stored][C][P], [upper slots][C][P], [C][P], [P]
	bool keep_partials = false;
	bool profiling = false;
	bool prof_pending = false, prof_with_upper = false;

	// the current tree's schedule under schedule_options (below), and the streamed walks' tables upload_schedule builds from it for
	// the current tile size; what runs on the walk lists is decided in "which kernel runs a pass"
	Schedule sched;
	Schedule sched_spare;  // the schedule the last phyamd_set_topology replaced: only its storage is used, by the next one
	StreamTables stream_tab;
	ScheduleCounts scaled_counts{0, 0, 1};  // those of the schedule a lazy rescaling switch would build (have_scaled_counts)
	bool have_scaled_counts = false;
	bool fusion_enabled = true;
	// (device copy of sched.deep_host: behind the tip-message table, see Ctx4::deep)

	// device memory
	DeviceArray<uint8_t> d_tipmask{&tile_mem};
	// 20 / 60 / 61 states: tip code S + 1 + q = ambiguity set q, one bit per member state (tip partials that are neither
	// one state nor all states: named sets of a general data type, states of a padded state space)
	DeviceArray<unsigned long long> d_tipsets{&mem};
	std::vector<unsigned long long> tipsets_host;
	size_t tipsets_uploaded = 0;  // entries of tipsets_host the device table holds
	DeviceArray<double> d_lower{&tile_mem}, d_upper{&tile_mem}, d_mats{&mem}, d_dmats{&mem};
	DeviceArray<double> d_Q{&mem};
	DeviceArray<double> d_Qpi{&mem};  // diag(pi) Q: the tree-walk gradient contracts u with (pi o Q b) in one mat-vec (4 states)
	std::vector<double> Q_host;
	bool have_Q = false;
	DeviceArray<double> d_tiptab{&mem};  // [T][C][16][4] tip messages (4-state), then the DeepDesc table
	// substitution-parameter gradient (G2)
	int np = 0;                      // number of dQ/dtheta matrices set
	std::vector<double> dQ_host;     // [np][S][S]
	DeviceArray<double> d_B{&mem};      // [np][S][S]  U^-1 dQ U
	DeviceArray<double> d_dpm{&mem};    // [np][N][C][S][S]
	DeviceArray<double> d_dptab{&mem};  // [np][T][C][16][4]
	DeviceArray<double> d_ppart{&mem};  // [np][upper ops][nblk] per-workgroup parameter sums, then [np][upper ops]
	DeviceArray<double> d_Bw{&mem};     // tree-walk G2: [np][16] U^-1 dQ U
	DeviceArray<double> d_pbuf{&mem};   // tree-walk G2: [UTpi 16 | Uinv 16 | utab 64]
	DeviceArray<double> d_Fw{&mem};     // tree-walk G2: [N][C][20] w_c F_ab(t_n r_c), l_a e^{l_a t_n r_c}
	DeviceArray<double> d_gacc{&mem};   // tree-walk G2: [16][slabs * C] per-wave eigen-basis sums, then [16] totals
	// phyamd_branch_log_likelihood without resident uppers: the one upper it needs is rebuilt by a root-to-node path walk
	DeviceArray<PathStep> d_path_steps{&mem};
	DeviceArray<double> d_path_upper{&mem}, d_path_tmp{&mem}, d_path_lower{&mem};  // one node partial each
	DeviceArray<double> d_path_side{&mem};  // 20 / 60 / 61 states: two node partials beside true_lower_gen (fused cherries below the node)
	DeviceArray<double> d_pg_lower{&mem};   // 20 / 60 / 61 states, parameter gradient: every stored node's partial itself (d_lower holds P p)
	// phyamd_branch_hessian_diagonal (ensure_hess_storage): workgroup table and slab of the HESS pre-order pass
	DeviceArray<int> d_hess_tab{&tile_mem};
	DeviceArray<double> d_hess{&tile_mem};
	int hess_nwg = 0, hess_P = -1, hess_levels = -1;
	DeviceArray<double> d_hess_invf{&mem};  // 20 / 60 / 61 states: 1 / pi [S]
	int gen_hess_slots[2] = {0, 0};  // resident workgroups of k_upper_gen<HESS> [SCALE]
	// how the last 20 / 60 / 61-state post-order and pre-order passes were launched (phyamd_get_general_profile): written by their launchers
	phyamd_general_profile gen_prof{-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	// which 4-state kernel the last post-order and pre-order passes launched (phyamd_get_pass_profile): written by their launchers
	// where they pick the instantiation (record_lower_pass, record_upper_pass), never by lower_kernel / upper_kernel
	phyamd_pass_profile pass_prof{-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
	DeviceArray<double> d_branch{&mem};  // phyamd_branch_log_likelihood: [C][3][16] matrices | [3][blocks] partial sums | [3]
	bool upper_fold = false;         // the stored uppers carry the root frequencies (last gradient call used FOLD)
	DeviceArray<double> d_rf_part{&mem};      // [S][blocks] partial sums of k_root_frequency_term, then [S]
	DeviceArray<double> d_gen_scratch{&mem};  // rescaled S != 4 path: per-level maxima / numerators / denominators
	// 20 / 60 / 61 states (k_param_*_gen): branch nodes, node -> stored lower index, per-branch site likelihoods, G tables
	DeviceArray<int> d_pg_nodes{&mem}, d_pg_core{&mem};
	DeviceArray<double> d_pg_den{&mem}, d_pg_Gw{&mem}, d_pg_B{&mem};
	DeviceArray<double> d_model{&mem}, d_freqs{&mem}, d_rates{&mem}, d_props{&mem}, d_lengths{&mem}, d_result{&mem};
	DeviceArray<double> d_weights{&tile_mem}, d_plk{&tile_mem}, d_lscale{&tile_mem}, d_lnl_part{&tile_mem}, d_gpart{&tile_mem};
	DeviceArray<double> d_wl{&tile_mem};  // [P] w_k / L_k from the root kernel (unscaled evaluations)
	DeviceArray<uint8_t> d_explicit{&mem}, d_row_valid{&mem};
	DeviceArray<NodeOp> d_lower_ops{&mem}, d_upper_ops{&mem};
	double *h_result = nullptr;  // pinned
	double *h_lengths = nullptr;  // pinned staging of phyamd_set_branch_lengths
	hipEvent_t ev_lengths = nullptr;
	hipEvent_t ev_check = nullptr;  // the lazy rescaling switch of a gradient call: lnL of the post-order pass is on its way to h_result's last entry
	bool check_pending = false;
	int nblk = 0;

	hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
	phyamd_profile prof{};

	// phyamd_gradient_batch, phyamd_gradient_batch_trees (phyamd_batch4.inc): op lists of the tree they were built for, and the
	// scratch of batch_items items -- per-item lengths, matrices and results; lowers, parked uppers and slabs; for a batch of trees
	// the items' own op lists and roots
	std::vector<uint8_t> tip_empty;      // tip -> some cell of its data has an empty state mask (0/1 tip partials that are all 0)
	int batch_max_patterns = 0;          // the fast path's pattern bound (BATCH_MAX_PATTERNS; PHYAMD_BATCH_MAX_PATTERNS: the crossover sweep)
	bool batch_trace = false;            // PHYAMD_BATCH_TRACE: a batch of trees reports each chunk's host times on stderr (profiles/tree_batch_timing.py)
	std::vector<int32_t> batch_left, batch_right;
	int batch_root = -1, batch_upper_slots = 0;
	std::vector<BatchOp> batch_ops;      // [post-order T - 1 | pre-order T - 1] of the engine's tree
	DeviceArray<BatchOp> d_batch_ops{&mem};
	// the scratch is a spare group of the shard's budget (DeviceBudget::spare): counted in device_bytes while held, released
	// whenever an array of the engine itself needs the room, with the pattern storage and on a new topology
	DeviceBudget batch_mem{&mem};
	DeviceArray<double> d_batch_len{&batch_mem}, d_batch_mats{&batch_mem}, d_batch_out{&batch_mem};
	DeviceArray<double> d_batch_lower{&batch_mem}, d_batch_upper{&batch_mem}, d_batch_slab{&batch_mem}, d_batch_lnl{&batch_mem};
	DeviceArray<BatchOp> d_batch_item_ops{&batch_mem};  // [item][post-order T - 1 | pre-order T - 1]
	DeviceArray<int32_t> d_batch_roots{&batch_mem};     // [item]
	// what the scratch holds: every call describes what it needs as a ScratchPlan (phyamd_queries.inc: batch_plan, reweight_plan,
	// nni_base_plan with nni_plan and cbopt_plan, nni_gen_plan, classcb_plan, blopt_plan, spr_plan with tripod_plan, spr_gen_plan with classgraft_plan, pairdist_plan, bhess_plan, sitelnl_plan; phyamd_place_calls.inc: place_plan,
	// place_gen_plan, qopt_plan, qopt_gen_plan) and gets at least that, so a call of one kind
	// never runs in the scratch of another with too few upper slots or without its lists.  batch_held: the plan the arrays were last
	// allocated by, for batch_items items (the Hessian's arrays, grown beside it, are judged by their sizes alone)
	ScratchPlan batch_held;
	size_t batch_items = 0;
	phyamd_batch_profile batch_prof{};
	// phyamd_nni_log_likelihoods (phyamd_nni4.inc) walks ONE item of the scratch above with every upper parked (slots = T - 1) and
	// adds to the group: the engine's tree's op lists in that form, the candidate edges and each node's candidate index, the trial
	// lengths and matrices, the slab and the result
	DeviceArray<BatchOp> d_nni_ops{&batch_mem};    // [post-order T - 1 | pre-order T - 1, every internal child's upper parked at child - T]
	DeviceArray<NniCand> d_nni_cands{&batch_mem};  // [T - 2]
	DeviceArray<int32_t> d_nni_cand_of{&batch_mem};  // [N]: node -> index in d_nni_cands, -1: a tip or the root
	DeviceArray<double> d_nni_len{&batch_mem}, d_nni_mats{&batch_mem};  // [3][N], [3][N][C][16]
	DeviceArray<double> d_nni_slab{&batch_mem}, d_nni_out{&batch_mem};  // [T - 2][blocks][9], [3 terms][3][N]
	bool nni_lists_valid = false;        // d_nni_ops, d_nni_cands and d_nni_cand_of hold the engine's tree's (while they are allocated)
	phyamd_nni_profile nni_prof{};
	// phyamd_nni_optimize (phyamd_nniopt4.inc) runs the same walk with the same lists (the start lengths go through d_nni_len) and
	// adds to the group, per candidate of a chunk: the coefficients of its three entries and their results
	DeviceArray<double> d_cbopt_K{&batch_mem};       // [candidate][3][C][4][blocks * 64]
	DeviceArray<double> d_cbopt_out{&batch_mem};     // [candidate][3][t*, lnL, d1, d2]
	DeviceArray<int32_t> d_cbopt_iter{&batch_mem};   // [candidate][3]
	phyamd_nni_optimize_profile cbopt_prof{};
	// phyamd_optimize_branch_lengths (phyamd_blopt4.inc) starts from the lnL-only walk of a batch of trees in the scratch above (the
	// items' lengths, matrices and lowers are its state) and adds to the group, per item: a plane O_n per node, the coefficients of
	// the branch being visited, the tour's ops and visit slots, the mask of visited nodes, lnL before and now, and the status words
	DeviceArray<double> d_blopt_O{&batch_mem};           // [item][N][C][blocks * 64][4]
	DeviceArray<double> d_blopt_K{&batch_mem};           // [item][C][4][blocks * 64]
	DeviceArray<BloptOp> d_blopt_ops{&batch_mem};        // [item][3 (T - 1)]
	DeviceArray<BloptVisit> d_blopt_visits{&batch_mem};  // [item][2 (T - 1)]
	DeviceArray<uint8_t> d_blopt_mask{&batch_mem};       // [item][N]
	DeviceArray<double> d_blopt_lnl{&batch_mem};         // [item][previous pass | now]
	DeviceArray<int32_t> d_blopt_status{&batch_mem};     // [item][BLOPT_STATUS]
	phyamd_branch_optimize_profile blopt_prof{};
	// phyamd_spr_log_likelihoods (phyamd_spr4.inc) walks one item of the scratch above per prune node (a ROW), with its own op
	// lists (d_batch_item_ops) and every upper parked (slots = T - 1), and adds to the group: per row the candidate edges, each
	// cell's candidate index, the slab and the result; once the engine's lengths with their halves and the matrices of both.
	// On the host: the engine's tree's park_all op lists, which every row's lists are a copy of but for the ghost, and each
	// node's interval in a depth-first numbering (n is in p's subtree: spr_tin[p] <= spr_tin[n] < spr_tout[p])
	std::vector<BatchOp> spr_ops;        // [post-order T - 1 | pre-order T - 1] (State::spr_lists_dirty)
	std::vector<int32_t> spr_tin, spr_tout, spr_lower_at, spr_upper_at;  // [N]; the index of an internal node's op in either list
	DeviceArray<SprCand> d_spr_cands{&batch_mem};    // [rows][at most N], the rows' candidates one after the other
	DeviceArray<int32_t> d_spr_cand_of{&batch_mem};  // [rows][N]: cell -> index in d_spr_cands, -1: no candidate
	DeviceArray<double> d_spr_slab{&batch_mem}, d_spr_out{&batch_mem};  // [candidate][blocks], [rows][N]
	DeviceArray<double> d_spr_len{&batch_mem}, d_spr_mats{&batch_mem};  // [t | 0.5 t][N], [2][N][C][16]
	phyamd_spr_profile spr_prof{};
	// phyamd_spr_optimize (phyamd_tripod4.inc) runs the same walk of the same rows with the same lists and adds to the group, per
	// candidate of a row: pi o U, the coefficients of the branch being visited, the result and the status words; per cell the
	// scattered results and counts
	DeviceArray<double> d_tripod_fU{&batch_mem};        // [candidate][C][blocks * 64][4]
	DeviceArray<double> d_tripod_K{&batch_mem};         // [candidate][C][4][blocks * 64]
	DeviceArray<double> d_tripod_res{&batch_mem};       // [candidate][t_p, t_w, t_u, lnl, initial_lnl]
	DeviceArray<int32_t> d_tripod_status{&batch_mem};   // [candidate][TRIPOD_STATUS]
	DeviceArray<double> d_tripod_out{&batch_mem};       // [rows][N][5]
	DeviceArray<int32_t> d_tripod_counts{&batch_mem};   // [rows][N][passes, visits, iterations]
	phyamd_spr_optimize_profile tripod_prof{};
	// phyamd_pairwise_distances (phyamd_pairdist4.inc) walks no tree: per pair of a chunk its two taxa, the record of the run of pairs
	// it shares its first taxon with, the segment sums of its 16 x 16 mask-pair table and the table, its start and its results.
	// phyamd_pairwise_distances_general (phyamd_pairdist_gen.inc) uses the same arrays with 32 x 32 class-pair tables: 1024 bins
	DeviceArray<int32_t> d_pairdist_pairs{&batch_mem}, d_pairdist_groups{&batch_mem};  // [pair][i, j], [group][first pair, pairs]
	DeviceArray<double> d_pairdist_part{&batch_mem};     // [segments][pair][256] ([1024])
	DeviceArray<double> d_pairdist_counts{&batch_mem};   // [pair][16 mi + mj] ([32 ci + cj])
	DeviceArray<double> d_pairdist_start{&batch_mem};    // [pair]
	DeviceArray<double> d_pairdist_out{&batch_mem};      // [pair][t*, lnL, d1, d2]
	DeviceArray<int32_t> d_pairdist_iter{&batch_mem};    // [pair]
	phyamd_distance_profile dist_prof{};
	// phyamd_placement_log_likelihoods (phyamd_place4.inc) runs the NNI call's walk (the split lengths go through d_nni_len, their
	// matrices through d_nni_mats) and adds to the group: the pendant lengths and their matrices, the edges, every query's best edge
	// so far, and per chunk of node columns and of queries the table, the caller's mask rows and their packed form, the slab and
	// the result
	DeviceArray<double> d_place_pend_len{&batch_mem}, d_place_pend{&batch_mem};  // [L], [L][C][16]
	DeviceArray<PlaceEdge> d_place_edges{&batch_mem};              // [N - 1]: the non-root nodes in node order
	DeviceArray<double> d_place_best_lnl{&batch_mem};              // [L][queries]
	DeviceArray<int32_t> d_place_best_node{&batch_mem};            // [L][queries]
	DeviceArray<double> d_place_table{&batch_mem};                 // [L][edges of the chunk][blocks * 64][16]
	DeviceArray<uint8_t> d_place_raw{&batch_mem};                  // [queries of the chunk][P]
	DeviceArray<unsigned long long> d_place_packed{&batch_mem};    // [blocks * 8][queries of the chunk]: eight patterns' masks per word
	DeviceArray<double> d_place_slab{&batch_mem};                  // [segments][L][edges of the chunk][queries of the chunk]
	DeviceArray<double> d_place_out{&batch_mem};                   // [L][queries of the chunk][node columns of the chunk]
	phyamd_placement_profile place_prof{};  // the last placement call of either kind
	// phyamd_placement_log_likelihoods_general (phyamd_place_gen.inc) reads the engine's resident partials and shares the 4-state
	// call's best edges, table, code rows, slab and result; it adds the lengths sigma t | (1 - sigma) t | pendant, their matrices
	// (and the derivatives the matrix kernel writes beside them), the images, the call's sets, and per node column of a chunk the
	// edge and its node's own partial
	DeviceArray<double> d_placeg_len{&batch_mem};                  // [2 N + L]
	DeviceArray<uint8_t> d_placeg_zero{&batch_mem};                // [2 N + L] zeros: no length has an explicit matrix
	DeviceArray<double> d_placeg_mats{&batch_mem}, d_placeg_dmats{&batch_mem};  // [2 N + L][C][400]
	DeviceArray<double> d_placeg_imgs{&batch_mem};                 // P_lo [N][C][image] | P_hi^T [N][C][image] | classes [L][C][640]
	DeviceArray<unsigned long long> d_placeg_sets{&batch_mem};     // [11]
	DeviceArray<PlaceGenEdge> d_placeg_edges{&batch_mem};          // [edges of the chunk]
	DeviceArray<double> d_placeg_own{&batch_mem};                  // [node columns of the chunk][C][20][Pp]
	DeviceArray<PlaceGenOwn> d_placeg_owns{&batch_mem};            // [internal nodes of the chunk]: what k_classplace_own forms each from
	// phyamd_placement_optimize (phyamd_qopt4.inc) runs the same walk and adds to the group, per chunk of candidates sorted by edge:
	// the chunk's distinct edges and pi o U of each, its distinct queries' mask rows, the candidates and their starts, the
	// coefficients of the branch being visited, the results and the status words
	DeviceArray<PlaceEdge> d_qopt_edges{&batch_mem};    // [edges of the chunk]
	DeviceArray<double> d_qopt_fU{&batch_mem};          // [edges of the chunk][C][blocks * 64][4]
	DeviceArray<uint8_t> d_qopt_masks{&batch_mem};      // [queries of the chunk][P]
	DeviceArray<QoptCand> d_qopt_cands{&batch_mem};     // [candidate]
	DeviceArray<double> d_qopt_start{&batch_mem};       // [candidate][t_n, t_x, t_z]
	DeviceArray<double> d_qopt_K{&batch_mem};           // [candidate][C][4][blocks * 64]
	DeviceArray<double> d_qopt_res{&batch_mem};         // [candidate][t_n, t_x, t_z, lnl, initial_lnl]
	DeviceArray<int32_t> d_qopt_status{&batch_mem};     // [candidate][QOPT_STATUS]
	phyamd_placement_optimize_profile qopt_prof{};  // the last placement-optimise call of either kind
	// phyamd_placement_optimize_general (phyamd_qopt_gen.inc) walks nothing: it reads the resident partials like
	// phyamd_placement_log_likelihoods_general and shares its sets and own partials (here: per distinct internal edge of a chunk) and
	// the 4-state call's code rows, starts, coefficients [candidate][C][20][Pp], results and status words; it adds its candidates
	DeviceArray<ClassOptCand> d_qoptg_cands{&batch_mem};  // [candidate]
	// phyamd_nni_log_likelihoods_general (phyamd_nni_gen.inc) walks nothing either: it reads the resident partials and the engine's
	// matrix images and shares the 4-state NNI call's candidate index, trial lengths, slab and result (d_nni_cand_of, d_nni_len,
	// d_nni_slab with blocks of 128 patterns, d_nni_out); it adds its candidates and the images of V^T and V^-1
	DeviceArray<ClassNniCand> d_nnig_cands{&batch_mem};   // [T - 2]
	DeviceArray<double> d_nnig_eig{&batch_mem};           // [V^T | V^-1][image]
	// phyamd_nni_optimize_general (phyamd_nniopt_gen.inc) reads the same partials through the same candidates, index and eigen images
	// (the start lengths go through d_nni_len) and adds, per candidate of a chunk: the coefficients of its three entries and their
	// results.  cbopt_prof keeps the last optimise call of either kind
	DeviceArray<double> d_classcb_K{&batch_mem};          // [candidate][3][C][20][Pp]
	DeviceArray<double> d_classcb_out{&batch_mem};        // [candidate][3][t*, lnL, d1, d2]
	DeviceArray<int32_t> d_classcb_iter{&batch_mem};      // [candidate][3]
	// phyamd_spr_log_likelihoods_general (phyamd_spr_gen.inc) reads the resident lowers and walks, per prune node of a chunk (a ROW),
	// the messages and uppers that pruning changes into the row's own planes.  It shares the 4-state SPR call's candidate index, slab
	// (blocks of 128 patterns) and result (d_spr_cand_of, d_spr_slab, d_spr_out) and host lists (spr_ops' pre-order, spr_tin, spr_tout),
	// and the placement call's lengths, matrices and images for the half lengths (d_placeg_len, _zero, _mats, _dmats, _imgs); it
	// adds the rows' ops, their counts, candidates and planes.  spr_prof keeps the last SPR scoring call of either kind
	DeviceArray<ClassSprOp> d_sprg_ops{&batch_mem};       // [row][T - 1 + path slots]
	DeviceArray<int32_t> d_sprg_nops{&batch_mem};         // [row]
	DeviceArray<ClassSprCand> d_sprg_cands{&batch_mem};   // [row][at most N], the rows' candidates one after the other
	DeviceArray<double> d_sprg_work{&batch_mem};          // [row][T - 1 uppers by internal node | path slots][C][20][Pp]
	// phyamd_spr_optimize_general (phyamd_graft_gen.inc) runs the same walk of the same rows with the same lists and shares the own-partial
	// records of the placement calls (d_placeg_owns), the starts of the placement optimiser (d_qopt_start: here t_p, t_w, t_u) and the
	// 4-state SPR optimiser's results, status words and scattered cells (d_tripod_res, _status, _out, _counts); it adds the own
	// partials, and per candidate of a row its record, pi o U and the coefficients of the branch being visited.  tripod_prof keeps
	// the last SPR optimise call of either kind
	DeviceArray<double> d_graft_own{&batch_mem};          // [T - 1 by internal node | row][path slots]: planes [C][20][Pp]
	DeviceArray<ClassGraftCand> d_graft_cands{&batch_mem};  // [row][at most N], the rows' candidates one after the other
	DeviceArray<double> d_graft_F{&batch_mem};            // [candidate][C][20][Pp]
	DeviceArray<double> d_graft_K{&batch_mem};            // [candidate][C][20][Pp]
	// phyamd_state_posteriors / phyamd_site_rate_posteriors (phyamd_post.inc): the rows of a chunk, their staged results -- [rows][P][S]
	// posteriors and [rows][P] states, or [P][C] + [P] site rates -- and, 20 / 60 / 61 states, each row's own partial p_n (true_lower_gen).
	// On demand, like d_branch: the calls read what the keep-partials gradient left and have no entry in the record above
	DeviceArray<PostRow> d_post_rows{&mem};
	DeviceArray<double> d_post_out{&mem}, d_post_lower{&mem};
	DeviceArray<uint8_t> d_post_states{&mem};
	// phyamd_branch_hessian (phyamd_bhess.inc): scratch of one chunk of whole 64-pattern blocks, held in the batch scratch's group --
	// counted in device_bytes while held, released with it (release_batch_scratch, a new topology, an array of the engine that needs
	// the room) and never assumed to hold anything: every call writes what it reads.  tan: the tangents [steps][C][Pc][4]; rows: w / L
	// and 1 / L [2][Pc], G [N][Pc], the walk's slab [steps + 2 N][blocks]; tiles: the cousin and the outer-product tiles
	// [tiles][blocks][256]; sums: the chunk's and the running matrix and gradient, r Q P and r^2 Q Q P; lists: the walk's starts and
	// steps, the tiles, each node's stored lower and upper.  Like the posteriors the call reads what the keep-partials gradient left
	// and has no entry in the record below: it leaves valid exactly what phyamd_state_posteriors leaves valid
	DeviceArray<double> d_bhess_tan{&batch_mem}, d_bhess_rows{&batch_mem}, d_bhess_tiles{&batch_mem}, d_bhess_sums{&batch_mem};
	DeviceArray<char> d_bhess_lists{&batch_mem};
	phyamd_hessian_profile bhess_prof{};
	// phyamd_gradient_batch_weights (phyamd_reweight.inc), in the batch scratch's group like the Hessian's arrays: a weight row per
	// item of a chunk ([items][P] beside the batched walk, [replicates][Pc] of a pattern chunk on the shared-lengths path), and on that
	// path the walk's rows R [1 + N C][Pc] and the replicates' segment sums [segments][replicates][rows].  The walk itself runs in
	// d_batch_lower / d_batch_upper and the results leave through d_batch_out
	DeviceArray<double> d_reweight_w{&batch_mem}, d_reweight_R{&batch_mem}, d_reweight_part{&batch_mem};
	// the engine's own weights on the host (shard_set_pattern_weights keeps them): a call that evaluates items with weights of
	// their own through the ordinary path puts these back.  weights_epoch: counts the uploads
	std::vector<double> weights_host;
	uint64_t weights_epoch = 0;
	phyamd_weight_batch_profile weight_prof{};
	// phyamd_pattern_log_likelihoods_trees (phyamd_sitelnl.inc) runs in the batch scratch's arrays: an item's lengths, matrices, op
	// list, root, per-block sums and lnL where a batch of trees has them, its few parked partials in d_batch_lower, its row of log L_k
	// in d_reweight_R, a replicate chunk's weight rows and segment sums in d_reweight_w and d_reweight_part; and adds the replicates'
	// results [replicates][items] of a chunk
	DeviceArray<double> d_sitelnl_rell{&batch_mem};
	phyamd_site_lnl_profile site_prof{};
};

// what the engine's schedule depends on besides its tree: the only place that derives it from an engine.  A caller that changes one
// of these switches rebuilds the schedule (rebuild_schedule, phyamd_eval.inc)
ScheduleOptions schedule_options(const Shard *e) {
	ScheduleOptions o;
	o.S = e->S;
	o.keep_partials = e->keep_partials;
	o.scaling_on = e->scaling_on;
	o.fusion_enabled = e->fusion_enabled;
	o.generic_fusion = e->generic_fusion;
	o.walk_enabled = e->walk_enabled;
	o.lower_park2_on = e->lower_park2_on;
	return o;
}

// ---- what each input invalidates -------------------------------------------------------------------------------------------
// The only place that writes Shard::state: a setter says which input changed (input_changed: the table), an evaluation what it has
// computed or overwritten (the transitions), and readers ask one of the three predicates.
enum class Input { TipData, PatternWeights, Topology, BranchLengths, BranchLength, Eigen, RateMatrix, Frequencies, CategoryRates, NodeMatrices,
                   Matrices, RateMatrixDerivatives, UpdateAllNodes, ScheduleRebuilt };

bool lowers_current(const Shard *e) { return !e->state.all_dirty && e->state.changed.empty() && !e->state.force_root; }
bool uppers_resident(const Shard *e) { return e->keep_partials && e->state.upper_valid; }
bool tiled_totals_current(const Shard *e, bool root_term = false) { return e->state.tiled_eval_done && (!root_term || e->state.tiled_root_term); }

// d_upper and d_path_upper belong to other lowers or have been overwritten / the stored lowers are not those of the current
// inputs, or not in the slots or the form their next reader needs: the next evaluation recomputes every node
void uppers_dropped(Shard *e) { e->state.upper_valid = false, e->state.path_node = -1; }
void lowers_discarded(Shard *e) { e->state.all_dirty = true, uppers_dropped(e); }

// input -> the products it invalidates.  node: the branch of BranchLength / NodeMatrices (-1: the node has none)
void input_changed(Shard *e, Input in, int node = -1) {
	Shard::State &s = e->state;
	s.tiled_eval_done = s.tiled_root_term = false;  // (every input: the totals are sums over what they were formed from)
	bool tables = false, lowers = false;            // P(t) with the tip tables / MFMA images; all lowers, and the uppers with them
	switch (in) {
	case Input::TipData: lowers = true, s.stored_valid = false, s.tip_epoch++; break;
	case Input::PatternWeights: lowers = true, s.stored_valid = false; break;
	case Input::Topology: tables = lowers = true, s.stored_valid = false, s.spr_lists_dirty = true, e->schedule_epoch++; break;  // (not part of phyamd_store)
	case Input::BranchLengths:  // the whole vector: every node is recomputed (SingleTreeLikelihood_update_all_nodes)
	case Input::CategoryRates:
	case Input::Matrices:
	case Input::UpdateAllNodes: tables = lowers = true; break;
	case Input::BranchLength:  // all P(t) are re-formed (microseconds); only the partials above `node` are recomputed
	case Input::NodeMatrices:
		tables = true, uppers_dropped(e);
		if (node >= 0) s.changed.push_back(node);
		break;
	case Input::Eigen: tables = lowers = true, s.qimg_dirty = s.qpi_dirty = s.params_dirty = true; break;
	case Input::RateMatrix: s.qimg_dirty = s.qpi_dirty = true; break;
	case Input::Frequencies: lowers = true, s.qimg_dirty = s.qpi_dirty = true; break;  // (20 / 60 / 61 states: the image of diag(pi) Q)
	case Input::RateMatrixDerivatives: s.params_dirty = true; break;
	case Input::ScheduleRebuilt: lowers = true, e->schedule_epoch++; break;  // slots start over: a stored state no longer maps onto them
	}
	if (tables) s.matrices_dirty = true;
	if (lowers) lowers_discarded(e);
}

// transitions: a tile's data are in place; the tails of run_lower, run_gradient and run_tiled (the resident partials are the last
// tile's only); shard_store; rebuild_path_upper; shard_restore's index flip (the root's outputs are still the discarded state's)
void tile_loaded(Shard *e) { e->state.tip_epoch++, lowers_discarded(e); }
void lowers_computed(Shard *e) { e->state.all_dirty = e->state.force_root = false, e->state.changed.clear(); }
void uppers_computed(Shard *e) { e->state.upper_valid = true; }
void tiled_totals_computed(Shard *e, bool root_term) { e->state.tiled_eval_done = true, e->state.tiled_root_term = root_term, lowers_discarded(e); }
void state_stored(Shard *e) { e->state.stored_valid = true; }
void path_upper_rebuilt(Shard *e, int node) { e->state.path_node = node; }
void lowers_restored(Shard *e) { lowers_computed(e), e->state.force_root = true; }
// a consumer has rebuilt its product: update_matrices (two), upload_qpi, ensure_tip_rate_products, the two uploads of U^-1 dQ U
void matrices_rebuilt(Shard *e) { e->state.matrices_dirty = false, e->state.qp_kind = -1; }
void q_images_rebuilt(Shard *e) { e->state.qimg_dirty = false, e->state.qp_kind = -1; }
void qpi_rebuilt(Shard *e) { e->state.qpi_dirty = false; }
void tip_rate_products_rebuilt(Shard *e, int kind) { e->state.qp_kind = kind; }
void parameter_basis_rebuilt(Shard *e) { e->state.params_dirty = false; }
void spr_lists_rebuilt(Shard *e) { e->state.spr_lists_dirty = false; }

// ---- what d_lower holds ----------------------------------------------------------------------------------------------------
// Every 4-state post-order pass records the form it wrote (launch_lower_w, launch_lower_stream).  A reader other than the two
// streamed walks settles the form before a pass is launched (require_reference_form, prefer_reference_form); launchers only check.

const char *form_name(LowerForm f) { return f == LowerForm::Reference ? "Reference" : f == LowerForm::Carried ? "Carried" : "CarriedExp2"; }

// the form the streamed post-order walk writes: t_n = P_n p_n -- rescaled: by powers of two per category -- unless a reader has
// needed the reference's (the reference's own rescaling, SCALE == 1, is by definition the reference's form)
LowerForm stream_lower_form(const Shard *e) {
	if (e->reference_form_only) return LowerForm::Reference;
	if (e->scaling_on) return e->exp2_on ? LowerForm::CarriedExp2 : LowerForm::Reference;
	return e->tform_on ? LowerForm::Carried : LowerForm::Reference;
}

// the streamed walks' instantiation (k_lower4_stream, k_upper4_stream) for stored lowers of form f in a pass with or without
// rescaling: SCALE (0: none, 1: the reference's, 2: powers of two) and TF.  scale = -1: no post-order pass writes f so
struct StreamVariant { int scale; bool tf; };
StreamVariant stream_variant(LowerForm f, bool scaling) {
	if (f != LowerForm::Reference && (f == LowerForm::CarriedExp2) != scaling) return {-1, false};
	return {f == LowerForm::CarriedExp2 ? 2 : scaling ? 1 : 0, f != LowerForm::Reference};
}

int check_reference_form(const Shard *e, const char *kernel) {  // a launcher of a kernel that reads the stored lowers as p_n
	if (e->lower_form == LowerForm::Reference) return PHYAMD_OK;
	return fail(PHYAMD_EDEVICE, "%s reads the stored lowers in the Reference form, they hold the %s form", kernel, form_name(e->lower_form));
}

int run_lower(Shard *e, int need_host_check);  // (phyamd_eval.inc)

// a reader needs the reference's form from the next post-order pass on (for good: the streamed walks lose their own forms)
void prefer_reference_form(Shard *e) { e->reference_form_only = true; }

// a reader needs the reference's form now: the post-order pass runs again if the stored lowers are in another form
int require_reference_form(Shard *e) {
	prefer_reference_form(e);
	if (e->lower_form == LowerForm::Reference) return PHYAMD_OK;
	lowers_discarded(e);
	return run_lower(e, 1);
}

// ---- which kernel runs a pass ----------------------------------------------------------------------------------------------
// A 4-state pass runs one of three families, and lower_kernel / upper_kernel below are the whole rule: the launchers launch the
// family they are given.
//            post-order        pre-order
//   Levels   k_lower4          k_upper4          one launch per tree level (phyamd_level4.inc)
//   Walk     k_lower4_walk     k_upper4_walk     the table-gather tree walks (phyamd_walk4.inc)
//   Stream   k_lower4_stream   k_upper4_stream   the streamed tree walks (phyamd_walk4s.inc)
// 20 states: the post-order pass is k_lower_gen_walk (Walk) or k_lower_gen (Levels); the 20 / 60 / 61-state pre-order pass and
// the branch Hessian's pass are always Levels.  A Stream answer holds once the walk's buffers are made (make_stream_buffers,
// then the same question with made = true): a cap may leave no room for them, and whether the tip data hold an empty state mask
// is known only once the mask words are built.
enum class PassKernel { Levels, Walk, Stream };

constexpr int STREAM_MAX_TIPS = 1 << 20;  // a packed mask-word entry keeps 20 bits of tip id

// the streamed walks can run on this engine: 4-state walk lists, few enough tips, and no cap has taken the pre-order walk's buffers
bool stream_possible(const Shard *e) { return e->sched.walking && e->T < STREAM_MAX_TIPS && !e->upper_stream_capped; }

// a streamed walk's workgroup holds the pass over stored lowers of form f: plain, rescaled by powers of two, or rescaled as the
// reference does (the C category waves of one block exchange their maxima: at most STREAM_WAVES of them)
bool stream_shape_fits(const Shard *e, LowerForm f) { return !e->scaling_on || f == LowerForm::CarriedExp2 || e->C <= STREAM_WAVES; }

// the post-order pass; a streamed one writes stream_lower_form
PassKernel lower_kernel(const Shard *e, bool made) {
	if (e->generic) return e->sched.gen_walking && !e->scaling_on && !e->incremental_pass ? PassKernel::Walk : PassKernel::Levels;
	const bool walk = e->sched.walking && !e->incremental_pass;
	if (walk && stream_possible(e) && !e->lower_stream_capped && stream_shape_fits(e, stream_lower_form(e)) && !e->stream_tab.lower_desc.empty() &&
	    !(made && e->stream_unsupported))
		return PassKernel::Stream;
	return walk ? PassKernel::Walk : PassKernel::Levels;
}

// the pre-order pass of a gradient (with_params: of the substitution-parameter gradient, the walk in its PARAMS form); the walks
// read the stored lowers in the form the post-order pass left
PassKernel upper_kernel(const Shard *e, int flags, bool with_params, bool made) {
	if (!e->sched.walking) return PassKernel::Levels;
	const bool compat = (flags & PHYAMD_GRAD_COMPAT_SCALED) && e->scaling_on;
	if (with_params) {  // the walk's eigen-basis branch term: explicit matrices have no eigen system; the compat arithmetic is the level kernels'
		const bool any_explicit = std::any_of(e->explicit_host.begin(), e->explicit_host.end(), [](uint8_t x) { return x != 0; });
		return any_explicit || compat ? PassKernel::Levels : PassKernel::Walk;
	}
	if (!compat && stream_possible(e) && stream_shape_fits(e, e->lower_form) && !(made && e->stream_unsupported)) return PassKernel::Stream;
	return PassKernel::Walk;
}

// ---- which path a batch takes (phyamd_gradient_batch, phyamd_gradient_batch_trees) -------------------------------------------
// The batched walk (k_batch_walk4) runs exactly when no condition of batch_walk_refusal holds.  For a batch of branch-length
// vectors it is an optimisation of "evaluate the items one by one": every other engine evaluates the items through the ordinary
// path (batch_fast_path).  A batch of trees has no such path to fall back to -- a loop over phyamd_set_topology rebuilds the
// schedule and discards the engine's partials per item -- and is refused with the condition's name (tree_batch_refusal).
// fit: items whose scratch fits the budget.

// the condition that keeps the batched walk off this engine, or null
const char *batch_walk_refusal(const Shard *e, int flags) {
	if (e->generic) return "the batched walk is built for 4 states";
	if (e->C > BATCH_MAX_CATEGORIES) return "the batched walk takes at most 8 categories (one LDS row per category)";
	if (e->scaling_on) return "the engine is rescaling and the batched walk does not rescale";
	if (e->tiles > 1) return "the patterns are tiled and the batched walk needs the tip data of all patterns resident";
	if (std::any_of(e->tip_empty.begin(), e->tip_empty.end(), [](uint8_t x) { return x != 0; })) return "a tip cell has an empty state mask";
	if (flags & ~PHYAMD_GRAD_FOLD_ROOT_FREQS) return "the batched walk takes flags 0 or PHYAMD_GRAD_FOLD_ROOT_FREQS";
	return nullptr;
}

// Above BATCH_MAX_PATTERNS patterns the loop over the single-evaluation walks wins: one evaluation fills the card by itself there,
// and those walks store half the partials (measured, profiles/batch_sweep.json, DESIGN.md "A batch of branch-length vectors": at
// 8 192 patterns the batched call is 2.1-3.6x faster at 64 taxa and between 1.2x faster and 1.3x slower at 500; at 32 768 the loop
// wins by up to 2.5x, but for a tie at 64 taxa x 32 items).
// 8 192 is a compromise, not a clean crossover: the point moves with the tree size and the batch size (profiles/batch_sweep.json).
constexpr int BATCH_MAX_PATTERNS = 8192;
bool batch_fast_path(const Shard *e, int flags, size_t fit) {
	if (batch_walk_refusal(e, flags)) return false;  // (RESCALE_AUTO: a non-finite item is redone through the ordinary path)
	if (e->P > e->batch_max_patterns) return false;
	return fit >= 1;
}

// a batch of trees: the walk's own conditions (no pattern bound: that one is a crossover against a loop that does not exist
// here), no explicit node matrices -- they belong to node ids of the engine's tree and cannot follow per-item lengths -- and
// scratch for at least one item.  RESCALE_AUTO: an item whose lnL is not finite is reported in-band; the engine is never switched
const char *tree_batch_refusal(const Shard *e, int flags, size_t fit) {
	if (const char *why = batch_walk_refusal(e, flags)) return why;
	if (std::any_of(e->explicit_host.begin(), e->explicit_host.end(), [](uint8_t x) { return x != 0; })) return "a node has explicit matrices, which cannot follow per-item trees and lengths";
	if (fit < 1) return "the scratch of one item does not fit the memory budget";
	return nullptr;
}
