// phycpp_amd/physher.hpp -- the C++ wrapper surface of physher's tree likelihood, MI355X-backed.
//
// Same class names, constructor arguments, method names and parameter/gradient orderings as the reference's
// src/phycpp/physher.hpp (the layer torchtree-physher binds), for the classes on the tree-likelihood path:
//   tree models      UnRootedTreeModelInterface, TimeTreeModelInterface, ReparameterizedTimeTreeModelInterface  (physher.hpp:127-174)
//   clock models     StrictClockModelInterface, SimpleClockModelInterface                                        (physher.hpp:176-199)
//   substitution     JC69Interface, HKYInterface, GTRInterface, GeneralSubstitutionModelInterface               (physher.hpp:201-267)
//   site models      Constant / Invariant / Weibull / Gamma SiteModelInterface                                  (physher.hpp:269-358)
//   likelihood       TreeLikelihoodInterface                                                                    (physher.hpp:360-395)
// The coalescent and CTMC-scale wrappers of the reference are priors, not part of this path, and are not provided.
// Behind TreeLikelihoodInterface sits the C ABI of include/physher_amd.h (HIP kernels); there is no CPU fallback.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <utility>
#include <vector>

namespace phyamd {
struct Tree;
struct SubstModel;
struct SiteModel;
struct DataType;
struct LikelihoodImpl;
}  // namespace phyamd

// bit values of the reference's TREELIKELIHOOD_FLAG_* (treelikelihood.h:32-38)
enum class TreeLikelihoodGradientFlags {
	TREE_HEIGHT = 1 << 0,
	SITE_MODEL = 1 << 1,
	SUBSTITUTION_MODEL = 1 << 2,
	SUBSTITUTION_MODEL_RATES = 1 << 3,
	SUBSTITUTION_MODEL_FREQUENCIES = 1 << 4,
	BRANCH_MODEL = 1 << 6
};

// treetransform.h:17-22
enum class TreeTransformFlags { RATIO = 1, SHIFT = 2, PROPORTION = 3 };

class DataTypeInterface {
   public:
	DataTypeInterface();
	virtual ~DataTypeInterface();
	std::shared_ptr<phyamd::DataType> dataType_;
};

class NucleotideDataTypeInterface : public DataTypeInterface {
   public:
	NucleotideDataTypeInterface();
};

class GeneralDataTypeInterface : public DataTypeInterface {
   public:
	GeneralDataTypeInterface(const std::vector<std::string> &states,
	                         std::optional<const std::map<std::string, std::vector<std::string>>> ambiguities);
};

class ModelInterface {
   public:
	virtual ~ModelInterface() = default;
	virtual void SetParameters(const double *parameters) = 0;
	virtual void GetParameters(double *parameters) = 0;
	size_t parameterCount_ = 0;
};

class CallableModelInterface : public ModelInterface {
   public:
	virtual double LogLikelihood() = 0;
	virtual void Gradient(double *gradient) = 0;
	size_t gradientLength_ = 0;
};

class TreeModelInterface : public ModelInterface {
   public:
	~TreeModelInterface() override;
	size_t GetNodeCount() { return nodeCount_; }
	size_t GetTipCount() { return tipCount_; }
	phyamd::Tree *GetTree() { return tree_.get(); }
	// version counter bumped on every change: the likelihood re-uploads branch lengths only when it moved
	unsigned long version_ = 0;
	std::vector<size_t> nodeMap_;

   protected:
	void InitializeMap(const std::vector<std::string> &taxa);
	std::unique_ptr<phyamd::Tree> tree_;
	size_t nodeCount_ = 0;
	size_t tipCount_ = 0;
};

class UnRootedTreeModelInterface : public TreeModelInterface {
   public:
	UnRootedTreeModelInterface(const std::string &newick, const std::vector<std::string> &taxa);
	// nodeCount - 2 branch lengths indexed by nodeMap_ (physher.cpp:51-64)
	void SetParameters(const double *parameters) override;
	void GetParameters(double *parameters) override;
};

class TimeTreeModelInterface : public TreeModelInterface {
   public:
	TimeTreeModelInterface(const std::string &newick, const std::vector<std::string> &taxa, const std::vector<double> dates);
	void SetParameters(const double *parameters) override;  // internal node heights by class id
	void GetParameters(double *parameters) override;
	virtual void GetNodeHeights(double *heights);
};

class ReparameterizedTimeTreeModelInterface : public TimeTreeModelInterface {
   public:
	ReparameterizedTimeTreeModelInterface(const std::string &newick, const std::vector<std::string> &taxa, const std::vector<double> dates,
	                                      TreeTransformFlags transform);
	void SetParameters(const double *parameters) override;  // ratios, root height at the root's class id
	void GetParameters(double *parameters) override;
	void GetNodeHeights(double *heights) override;
	void GradientTransformJVP(double *gradient, const double *height_gradient);
	void GradientTransformJVP(double *gradient, const double *height_gradient, const double *heights);
	void GradientTransformJacobian(double *gradient);
	double TransformJacobian();
};

class BranchModelInterface : public ModelInterface {
   public:
	void SetParameters(const double *parameters) override;
	void GetParameters(double *parameters) override;
	void SetRates(const double *rates);
	// rate of the branch above node `id`
	double Rate(size_t node_id) const;
	std::vector<double> rates_;
	std::vector<size_t> map_;  // node id -> index into rates_ (strict clock: all 0)
	unsigned long version_ = 0;

   protected:
	TreeModelInterface *treeModel_ = nullptr;
};

class StrictClockModelInterface : public BranchModelInterface {
   public:
	StrictClockModelInterface(double rate, TreeModelInterface *treeModel);
	void SetRate(double rate);
};

class SimpleClockModelInterface : public BranchModelInterface {
   public:
	SimpleClockModelInterface(const std::vector<double> &rates, TreeModelInterface *treeModel);
};

class SubstitutionModelInterface : public ModelInterface {
   public:
	~SubstitutionModelInterface() override;
	DataTypeInterface *GetDataType() { return dataType_; }
	phyamd::SubstModel *GetModel() { return substModel_.get(); }
	unsigned long version_ = 0;

   protected:
	std::unique_ptr<phyamd::SubstModel> substModel_;
	DataTypeInterface *dataType_ = nullptr;
	bool ownsDataType_ = false;
};

class JC69Interface : public SubstitutionModelInterface {
   public:
	JC69Interface();
	void SetParameters(const double *parameters) override {}
	void GetParameters(double *parameters) override {}
};

class HKYInterface : public SubstitutionModelInterface {
   public:
	HKYInterface(double kappa, const std::vector<double> &frequencies);
	void SetKappa(double kappa);
	void SetFrequencies(const double *frequencies);
	void SetParameters(const double *parameters) override;
	void GetParameters(double *parameters) override {}
};

class GTRInterface : public SubstitutionModelInterface {
   public:
	GTRInterface(const std::vector<double> &rates, const std::vector<double> &frequencies);
	void SetRates(const double *rates);
	void SetFrequencies(const double *frequencies);
	void SetParameters(const double *parameters) override;
	void GetParameters(double *parameters) override {}
};

class GeneralSubstitutionModelInterface : public SubstitutionModelInterface {
   public:
	GeneralSubstitutionModelInterface(DataTypeInterface *dataType, const std::vector<double> &rates, const std::vector<double> &frequencies,
	                                  const std::vector<unsigned> &mapping, bool normalize);
	void SetRates(const double *rates);
	void SetFrequencies(const double *frequencies);
	void SetParameters(const double *parameters) override;
	void GetParameters(double *parameters) override {}
};

class SiteModelInterface : public ModelInterface {
   public:
	~SiteModelInterface() override;
	void SetMu(double mu);
	virtual void GetRates(double *rates);
	virtual void GetProportions(double *proportions);
	void SetParameters(const double *parameters) override;  // [shape] [pinv] [mu], whichever exist (physher.cpp:504-519)
	void GetParameters(double *parameters) override;
	phyamd::SiteModel *GetModel() { return siteModel_.get(); }
	unsigned long version_ = 0;

   protected:
	std::unique_ptr<phyamd::SiteModel> siteModel_;
};

class ConstantSiteModelInterface : public SiteModelInterface {
   public:
	explicit ConstantSiteModelInterface(std::optional<double> mu);
	void GetRates(double *rates) override;  // includes mu (physher.cpp:393-395)
};

class InvariantSiteModelInterface : public SiteModelInterface {
   public:
	InvariantSiteModelInterface(double proportionInvariant, std::optional<double> mu);
	void SetProportionInvariant(double value);
};

class DiscretizedSiteModelInterface : public SiteModelInterface {
   public:
	void SetParameter(double parameter);
	void SetProportionInvariant(double value);
	size_t GetCategoryCount() { return categoryCount_; }

   protected:
	DiscretizedSiteModelInterface(int distribution, double shape, size_t categories, std::optional<double> proportionInvariant,
	                              std::optional<double> mu);
	size_t categoryCount_ = 1;
};

class WeibullSiteModelInterface : public DiscretizedSiteModelInterface {
   public:
	WeibullSiteModelInterface(double shape, size_t categories, std::optional<double> proportionInvariant, std::optional<double> mu);
	void SetShape(double shape);
};

class GammaSiteModelInterface : public DiscretizedSiteModelInterface {
   public:
	GammaSiteModelInterface(double shape, size_t categories, std::optional<double> proportionInvariant, std::optional<double> mu);
	void SetShape(double shape);
	void SetEpsilon(double epsilon);
	double epsilon_ = 1.e-6;
};

class TreeLikelihoodInterface : public CallableModelInterface {
   public:
	TreeLikelihoodInterface(const std::vector<std::pair<std::string, std::string>> &alignment, TreeModelInterface *treeModel,
	                        SubstitutionModelInterface *substitutionModel, SiteModelInterface *siteModel,
	                        std::optional<BranchModelInterface *> branchModel, bool use_ambiguities = false, bool use_tip_states = false,
	                        bool include_jacobian = false);
	// one attribute (state name) per taxon: discrete-trait likelihoods (physher.hpp:369-377, new_AttributePattern)
	TreeLikelihoodInterface(const std::vector<std::string> &taxa, const std::vector<std::string> &attributes, TreeModelInterface *treeModel,
	                        SubstitutionModelInterface *substitutionModel, SiteModelInterface *siteModel,
	                        std::optional<BranchModelInterface *> branchModel, bool use_ambiguities = false, bool use_tip_states = false,
	                        bool include_jacobian = false);
	~TreeLikelihoodInterface() override;

	void RequestGradient(std::vector<TreeLikelihoodGradientFlags> flags = std::vector<TreeLikelihoodGradientFlags>());
	double LogLikelihood() override;
	void Gradient(double *gradient) override;
	void SetParameters(const double *parameters) override {}
	void GetParameters(double *parameters) override {}
	void EnableSSE(bool flag) {}  // CPU kernel switch of the reference (physher.cpp:662-665): no meaning on the GPU path

	// --- beyond the reference surface ---
	// reproduce the reference's include_root_freqs = true / rescaled-gradient arithmetic bit for bit ("quirks")
	void SetReferenceCompatibility(bool on) { referenceCompat_ = on; }
	// lnL / lnL and the gradient for `count` parameter vectors of the tree model at once (one phyamd_gradient_batch call):
	// treeParameters [count][n] is what the tree model's SetParameters takes -- branch lengths for unrooted trees, heights or
	// ratios + root height for time trees (clock rates are folded in as for a single evaluation); logLikelihoods [count] is
	// LogLikelihood() per item (may be null in GradientBatch); gradients [count][gradientLength_] is Gradient() per item: the
	// TREE_HEIGHT block and, when requested, the BRANCH_MODEL block, in Gradient's order, with the ratio transform's Jacobian
	// when the object includes it.  A request with SITE_MODEL or substitution-model flags throws.  The tree model holds its
	// previous parameters afterwards.  With SetReferenceCompatibility(true) gradients are the reference's arithmetic, which the
	// engine evaluates item by item (never batched); lnL is batched either way.
	void LogLikelihoodBatch(size_t count, const double *treeParameters, double *logLikelihoods);
	void GradientBatch(size_t count, const double *treeParameters, double *logLikelihoods, double *gradients);
	// lnL and the gradient for `count` pattern-weight vectors at once (one phyamd_gradient_batch_weights call): bootstrap or
	// jackknife replicates, RELL reweighting, site minibatches.  weights [count][patterns] in this object's pattern order
	// (PatternWeights() is the alignment's own row), finite and >= 0; treeParameters [count][n] as in GradientBatch, or null:
	// every item on the tree model's current parameters, which one walk of the tree then serves.  logLikelihoods (may be null)
	// and gradients are GradientBatch's, item b being what Gradient() returns with weights[b] as the pattern weights; the same
	// requests throw.  This object's own weights and the tree model's parameters are unchanged afterwards.
	void GradientWeights(size_t count, const double *weights, const double *treeParameters, double *logLikelihoods, double *gradients);
	// lnL / lnL and the branch gradient of `count` TREES on this object's alignment and models at once (one
	// phyamd_gradient_batch_trees call): left, right [count][2T-1] and roots [count] are plain node-id arrays, tips 0..T-1 in this
	// object's taxon order (the tree model's tip ids), internal ids T..2T-2 in any order, -1 / -1 for tips; branchLengths
	// [count][2T-1] by the item's node ids (root entry ignored); logLikelihoods [count] (may be null in GradientTrees);
	// branchGradients [count][2T-1] is d lnL / d length by the item's node ids (the root's entry 0), formed from the per-category
	// gradient as Gradient() does.  Only branch lengths are differentiated: a time-tree model (node heights) or a request with
	// BRANCH_MODEL, SITE_MODEL or substitution-model flags throws.  The tree model and this object's own state are unchanged.
	void LogLikelihoodTrees(size_t count, const int32_t *left, const int32_t *right, const int32_t *roots, const double *branchLengths, double *logLikelihoods);
	void GradientTrees(size_t count, const int32_t *left, const int32_t *right, const int32_t *roots, const double *branchLengths, double *logLikelihoods,
	                   double *branchGradients);
	// Beyond the reference surface: the per-pattern log-likelihoods of `count` TREES at once, and RELL replicates of them (one
	// phyamd_pattern_log_likelihoods_trees call; see include/physher_amd.h): the arrays are LogLikelihoodTrees'; logLikelihoods
	// [count]; patternLogLikelihoods [count][patterns] in this object's pattern order, or null; replicateWeights
	// [replicateCount][patterns], finite and >= 0, with replicateLogLikelihoods [replicateCount][count], or 0 and both null.  The
	// tree model and this object's own state are unchanged.
	void PatternLogLikelihoodsTrees(size_t count, const int32_t *left, const int32_t *right, const int32_t *roots, const double *branchLengths, double *logLikelihoods,
	                                double *patternLogLikelihoods, size_t replicateCount, const double *replicateWeights, double *replicateLogLikelihoods);
	// lnL and its first two derivatives in the central branch for every NNI neighbour of the tree model's tree at once (one
	// phyamd_nni_log_likelihoods call; see include/physher_amd.h for the candidates and the three arrangements): logLikelihoods,
	// d1, d2 [3][2T-1] by the tree's node ids, NaN at tips and the root; centralLengths [3][2T-1] trial lengths of the central
	// branch, or null for the branch's own.  Lengths and derivatives are in the engine's branch lengths (what a single
	// evaluation hands it: the tree model's lengths, with a clock rate or mu folded in).  d1 and d2 may be null.  The tree model
	// and this object's own state are unchanged.
	void NNILogLikelihoods(const double *centralLengths, double *logLikelihoods, double *d1, double *d2);
	// The same for a model of 20 states (one phyamd_nni_log_likelihoods_general call; see include/physher_amd.h): the arrays are
	// NNILogLikelihoods'.  The call reads the engine's resident partials, which it makes resident if they are not; the tree model
	// and this object's own state are unchanged.
	void NNILogLikelihoodsGeneral(const double *centralLengths, double *logLikelihoods, double *d1, double *d2);
	// The central branch of every NNI neighbour of the tree model's tree optimised at once (one phyamd_nni_optimize call; see
	// include/physher_amd.h for the rule): lengths, logLikelihoods, d1, d2 and iterations [3][2T-1] by the tree's node ids, in
	// NNILogLikelihoods' rows and columns (NaN, iterations 0, at tips and the root); startLengths [3][2T-1], or null for the
	// branch's own length; the optimum is sought in [lower, upper] until a step is no longer than tolerance, in at most
	// maxIterations steps (an entry that runs out of them, or whose lnL is not finite, has a negative count).  Lengths and
	// derivatives are in the engine's branch lengths, as for NNILogLikelihoods.  d1, d2 and iterations may be null.  The tree
	// model and this object's own state are unchanged.
	void NNIOptimize(const double *startLengths, double lower, double upper, double tolerance, int maxIterations, double *lengths, double *logLikelihoods, double *d1,
	                 double *d2, int32_t *iterations);
	// The same for a model of 20 states (one phyamd_nni_optimize_general call; see include/physher_amd.h): the arguments and arrays
	// are NNIOptimize's.  The call reads the engine's resident partials, which it makes resident if they are not; the tree model
	// and this object's own state are unchanged.
	void NNIOptimizeGeneral(const double *startLengths, double lower, double upper, double tolerance, int maxIterations, double *lengths, double *logLikelihoods,
	                        double *d1, double *d2, int32_t *iterations);
	// Every branch length of `count` TREES optimised on the device, one branch at a time, pass after pass (one
	// phyamd_optimize_branch_lengths call; see include/physher_amd.h for the rule): left, right, roots and branchLengths are
	// LogLikelihoodTrees' arrays, branchLengths the start; optimise [count][2T-1] marks the nodes whose branches are visited, or null:
	// every node but the root.  A visit seeks its branch's optimum in [lower, upper] until a step is no longer than tolerance, in at
	// most maxIterations steps; an item stops when a pass gains no more than lnlTolerance, or after maxPasses passes.  lengths
	// [count][2T-1] by the item's node ids, logLikelihoods [count]; initialLogLikelihoods [count] and passes [count] (negative: the
	// passes ran out, or lnL was not finite) may be null.  Lengths are the engine's branch lengths, as for NNILogLikelihoods.  The
	// tree model and this object's own state are unchanged.
	void OptimizeBranchLengths(size_t count, const int32_t *left, const int32_t *right, const int32_t *roots, const double *branchLengths, const uint8_t *optimise,
	                           double lower, double upper, double tolerance, int maxIterations, double lnlTolerance, int maxPasses, double *lengths,
	                           double *logLikelihoods, double *initialLogLikelihoods, int32_t *passes);
	// lnL of every SPR regraft of `count` prune nodes of the tree model's tree at once (one phyamd_spr_log_likelihoods call; see
	// include/physher_amd.h for the move and the candidates): out [count][2T-1] by the tree's node ids, row i the prune node
	// prune[i] (null: count = 2T-1 and row i is node i), column w the target edge; NaN where there is no candidate.  Lengths are
	// the engine's branch lengths, as for NNILogLikelihoods.  The tree model and this object's own state are unchanged.
	void SPRLogLikelihoods(const int *prune, int count, double *out);
	// The same for a model of 20 states (one phyamd_spr_log_likelihoods_general call; see include/physher_amd.h): the arguments and
	// the array are SPRLogLikelihoods'.  The call reads the engine's resident partials, which it makes resident if they are not;
	// the tree model and this object's own state are unchanged.
	void SPRLogLikelihoodsGeneral(const int *prune, int count, double *out);
	// The three branches that meet at the graft point of every SPR regraft optimised at once (one phyamd_spr_optimize call; see
	// include/physher_amd.h for the rule): SPRLogLikelihoods' rows, columns and candidates; lengths [count][2T-1][3] holds the lengths
	// of the prune node, of the target node and of the prune node's parent, logLikelihoods [count][2T-1]; initialLogLikelihoods
	// [count][2T-1] and passes [count][2T-1] (negative: the passes ran out, or lnL was not finite) may be null; NaN and 0 where there is
	// no candidate.  A visit seeks its branch's optimum in [lower, upper] until a step is no longer than tolerance, in at most
	// maxIterations steps; an entry stops when a pass gains no more than lnlTolerance, or after maxPasses passes.  Lengths are the
	// engine's branch lengths, as for NNILogLikelihoods.  The tree model and this object's own state are unchanged.
	void SPROptimize(const int *prune, int count, double lower, double upper, double tolerance, int maxIterations, double lnlTolerance, int maxPasses, double *lengths,
	                 double *logLikelihoods, double *initialLogLikelihoods, int32_t *passes);
	// The same for a model of 20 states (one phyamd_spr_optimize_general call; see include/physher_amd.h): the arguments and arrays are
	// SPROptimize's, the rows, columns and candidates SPRLogLikelihoodsGeneral's.  The call reads the engine's resident partials, which
	// it makes resident if they are not; the tree model and this object's own state are unchanged.
	void SPROptimizeGeneral(const int *prune, int count, double lower, double upper, double tolerance, int maxIterations, double lnlTolerance, int maxPasses,
	                        double *lengths, double *logLikelihoods, double *initialLogLikelihoods, int32_t *passes);
	// Beyond the reference surface: the maximum-likelihood distance of `count` pairs of taxa under this object's own models, before
	// any tree is scored (one phyamd_pairwise_distances call; see include/physher_amd.h for the definition and the rule): pairs
	// [count][2] holds two tip ids of the tree model each (null: count = T(T-1)/2, all i < j row-major); start [count] may be null
	// (0.1).  distances [count]; logLikelihoods, d1, d2 and iterations [count] may be null; counts [count][16][16], if not null,
	// receives the weighted tables of state-mask pairs.  With distances null and counts given the call only counts.  The tree
	// model and this object's own state are unchanged.
	void PairwiseDistances(const int *pairs, int count, const double *start, double lower, double upper, double tolerance, int maxIterations, double *distances,
	                       double *logLikelihoods, double *d1, double *d2, int32_t *iterations, double *counts);
	// The same for a data type of 20 states (one phyamd_pairwise_distances_general call; see include/physher_amd.h for the classes):
	// counts [count][32][32], if not null, receives the weighted tables of tip-class pairs, and classMembers [32], if not null, one
	// bit per member state of each class -- the classes of ambiguity sets are numbered by the engine, so classMembers is what
	// gives counts its meaning.
	void PairwiseDistancesGeneral(const int *pairs, int count, const double *start, double lower, double upper, double tolerance, int maxIterations, double *distances,
	                              double *logLikelihoods, double *d1, double *d2, int32_t *iterations, double *counts, uint64_t *classMembers);
	// Beyond the reference surface: lnL of `queries` sequences that are not among the tree model's taxa, each placed on every edge
	// of its tree (one phyamd_placement_log_likelihoods call; see include/physher_amd.h for the definition): masks
	// [queries][patterns] holds a 4-bit state mask 1..15 per query and pattern over THIS OBJECT'S OWN PATTERNS (GetPatternCount(); the
	// reference and the queries are compressed jointly, or not at all), pendant [lengths] the pendant lengths, split the part of
	// an edge's length that stays below the new node.  logLikelihoods [lengths][queries][2T-1] by the tree's node ids, NaN in the
	// root's column; bestNodes and bestLogLikelihoods [lengths][queries]: the smallest node id with the largest lnL, and that lnL.
	// logLikelihoods or bestNodes may be null, bestLogLikelihoods only needs bestNodes.  Lengths are the engine's branch lengths,
	// as for NNILogLikelihoods.  The tree model and this object's own state are unchanged.
	void PlacementLogLikelihoods(const uint8_t *masks, int queries, const double *pendant, int lengths, double split, double *logLikelihoods, int32_t *bestNodes,
	                             double *bestLogLikelihoods);
	// The same for a data type of 20 states (one phyamd_placement_log_likelihoods_general call; see include/physher_amd.h for the
	// classes): codes [queries][patterns] holds a class code per query and pattern -- 0..19 a state, 20 unknown, 21 + q the set
	// sets[q] of this call (bit s = state s is a member; setCount <= 11, sets may be null with setCount 0).  The outputs are
	// PlacementLogLikelihoods'.  The engine behind this object keeps every partial resident from here on; the tree model is unchanged.
	void PlacementLogLikelihoodsGeneral(const uint8_t *codes, int queries, const uint64_t *sets, int setCount, const double *pendant, int lengths, double split,
	                                    double *logLikelihoods, int32_t *bestNodes, double *bestLogLikelihoods);
	// The three branches around chosen placements optimised at once (one phyamd_placement_optimize call; see include/physher_amd.h
	// for the rule): masks and queries as for PlacementLogLikelihoods; candidates [count][2] holds (query, node) pairs by the tree's
	// node ids; pendantStart [count] may be null (0.1); split as there; branches marks what is optimised (bit 0: the node's branch
	// below the new node, bit 1: the query's, bit 2: the new node's; 7: all three).  lengths [count][3] holds those three in that
	// order, logLikelihoods [count]; initialLogLikelihoods [count] and passes [count] (negative: the passes ran out, or lnL was not
	// finite) may be null.  The bounds, tolerances and counts are SPROptimize's.  Lengths are the engine's branch lengths, as for
	// NNILogLikelihoods.  The tree model and this object's own state are unchanged.
	void PlacementOptimize(const uint8_t *masks, int queries, const int32_t *candidates, int count, const double *pendantStart, double split, int branches, double lower,
	                       double upper, double tolerance, int maxIterations, double lnlTolerance, int maxPasses, double *lengths, double *logLikelihoods,
	                       double *initialLogLikelihoods, int32_t *passes);
	// The same for a data type of 20 states (one phyamd_placement_optimize_general call; see include/physher_amd.h for the rule in
	// full): codes, sets and setCount as for PlacementLogLikelihoodsGeneral, everything else as for PlacementOptimize.  The engine
	// behind this object keeps every partial resident from here on; the tree model is unchanged.
	void PlacementOptimizeGeneral(const uint8_t *codes, int queries, const uint64_t *sets, int setCount, const int32_t *candidates, int count, const double *pendantStart,
	                              double split, int branches, double lower, double upper, double tolerance, int maxIterations, double lnlTolerance, int maxPasses,
	                              double *lengths, double *logLikelihoods, double *initialLogLikelihoods, int32_t *passes);
	// Beyond the reference surface: marginal ancestral reconstruction of `count` nodes of the tree model's tree at once (one
	// phyamd_state_posteriors call; see include/physher_amd.h for the definition): posteriors [count][patterns][states] and states
	// [count][patterns] by the tree's node ids, row i the node nodes[i] (null: count = 2T-1 and row i is node i; tips and the
	// root included), patterns in this object's pattern order.  Either output may be null.  The engine behind this object keeps
	// every partial resident from here on; the tree model is unchanged.
	void StatePosteriors(const int *nodes, int count, double *posteriors, unsigned char *states);
	// Beyond the reference surface: the posterior of each pattern's rate category, posteriors [patterns][categories], and its mean
	// rate, meanRates [patterns] or null (one phyamd_site_rate_posteriors call).
	void SiteRatePosteriors(double *posteriors, double *meanRates);
	// Beyond the reference surface: the full branch-length Hessian of lnL at the tree model's lengths (one phyamd_branch_hessian
	// call; see include/physher_amd.h for the definition): hessian [2T-1][2T-1] and gradient [2T-1] (or null) by the tree's node
	// ids, in the engine's branch lengths like NNILogLikelihoods; the root's row and column are 0, and the unrooted-tree epilogue
	// (the row of the root's child whose length is not a parameter) is the caller's.  Returns lnL.  The engine behind this object
	// keeps every partial resident from here on; the tree model is unchanged.
	double BranchHessian(double *gradient, double *hessian);
	size_t StateCount() const;
	size_t CategoryCount() const;
	size_t NodeCount() const;  // 2T - 1
	size_t TreeParameterCount() const { return treeModel_->parameterCount_; }  // n of treeParameters [count][n]
	size_t GetPatternCount() const;
	const std::vector<double> &PatternWeights() const;
	const std::vector<unsigned char> &PatternStates() const;  // [taxon][pattern], taxa in alignment order

   private:
	void Init(bool use_tip_states);
	void Sync();
	void FormBranchLengths(std::vector<double> &lengths);
	void GradientEpilogue(double lnl, std::vector<double> &cat_grad, const std::vector<double> &branch_lengths, const std::vector<double> &subst_grad,
	                      double *gradient);
	void EvaluateBatch(size_t count, const double *treeParameters, double *logLikelihoods, double *gradients, const double *weights);
	void BranchGradientFromCat(const double *cat_grad, double *g);
	void EvaluateTrees(size_t count, const int32_t *left, const int32_t *right, const int32_t *roots, const double *branchLengths, double *logLikelihoods,
	                   double *branchGradients);
	TreeModelInterface *treeModel_;
	SubstitutionModelInterface *substitutionModel_;
	SiteModelInterface *siteModel_;
	BranchModelInterface *branchModel_;
	bool includeJacobian_;
	bool referenceCompat_ = false;
	int flags_ = 0;
	bool substRates_ = false, substFreqs_ = false;
	std::unique_ptr<phyamd::LikelihoodImpl> impl_;
};
