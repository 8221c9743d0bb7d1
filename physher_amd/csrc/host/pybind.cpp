// pybind.cpp -- Python module over the phycpp-compatible classes (the role torchtree-physher's binding plays for
// the reference's src/phycpp).  Arrays cross as numpy float64; nothing is computed here.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "phyamd_host.hpp"
#include "phycpp_amd/physher.hpp"

namespace py = pybind11;
using darray = py::array_t<double, py::array::c_style | py::array::forcecast>;

static darray vec(const std::vector<double> &v) { return darray(v.size(), v.data()); }
using iarray = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;

// shapes of a batch of trees: left, right, lengths [count][2T-1], roots [count]; returns count
static size_t check_trees(const TreeLikelihoodInterface &tlk, const iarray &left, const iarray &right, const iarray &roots, const darray &lengths) {
	const py::ssize_t N = (py::ssize_t)tlk.NodeCount();
	if (left.ndim() != 2 || left.shape(1) != N) throw phyamd::Error("left: [count][node_count]");
	const py::ssize_t count = left.shape(0);
	if (right.ndim() != 2 || right.shape(0) != count || right.shape(1) != N) throw phyamd::Error("right: [count][node_count]");
	if (roots.ndim() != 1 || roots.shape(0) != count) throw phyamd::Error("roots: [count]");
	if (lengths.ndim() != 2 || lengths.shape(0) != count || lengths.shape(1) != N) throw phyamd::Error("branch lengths: [count][node_count]");
	return (size_t)count;
}

PYBIND11_MODULE(_phycpp_amd, m) {
	m.doc() = "phycpp-compatible host classes over the MI355X tree-likelihood engine";
	py::register_exception<phyamd::Error>(m, "PhyamdError");

	py::enum_<TreeLikelihoodGradientFlags>(m, "TreeLikelihoodGradientFlags")
	    .value("TREE_HEIGHT", TreeLikelihoodGradientFlags::TREE_HEIGHT)
	    .value("SITE_MODEL", TreeLikelihoodGradientFlags::SITE_MODEL)
	    .value("SUBSTITUTION_MODEL", TreeLikelihoodGradientFlags::SUBSTITUTION_MODEL)
	    .value("SUBSTITUTION_MODEL_RATES", TreeLikelihoodGradientFlags::SUBSTITUTION_MODEL_RATES)
	    .value("SUBSTITUTION_MODEL_FREQUENCIES", TreeLikelihoodGradientFlags::SUBSTITUTION_MODEL_FREQUENCIES)
	    .value("BRANCH_MODEL", TreeLikelihoodGradientFlags::BRANCH_MODEL);
	py::enum_<TreeTransformFlags>(m, "TreeTransformFlags")
	    .value("RATIO", TreeTransformFlags::RATIO)
	    .value("SHIFT", TreeTransformFlags::SHIFT)
	    .value("PROPORTION", TreeTransformFlags::PROPORTION);

	py::class_<DataTypeInterface>(m, "DataTypeInterface");
	py::class_<NucleotideDataTypeInterface, DataTypeInterface>(m, "NucleotideDataTypeInterface").def(py::init<>());
	py::class_<GeneralDataTypeInterface, DataTypeInterface>(m, "GeneralDataTypeInterface")
	    .def(py::init<const std::vector<std::string> &, std::optional<const std::map<std::string, std::vector<std::string>>>>(), py::arg("states"),
	         py::arg("ambiguities") = py::none());

	py::class_<ModelInterface>(m, "ModelInterface")
	    .def_readonly("parameter_count", &ModelInterface::parameterCount_)
	    .def("set_parameters", [](ModelInterface &self, darray p) { self.SetParameters(p.data()); })
	    .def("get_parameters", [](ModelInterface &self) {
		    std::vector<double> v(self.parameterCount_);
		    self.GetParameters(v.data());
		    return vec(v);
	    });
	py::class_<CallableModelInterface, ModelInterface>(m, "CallableModelInterface")
	    .def_readonly("gradient_length", &CallableModelInterface::gradientLength_)
	    .def("log_likelihood", &CallableModelInterface::LogLikelihood)
	    .def("gradient", [](CallableModelInterface &self) {
		    std::vector<double> g(self.gradientLength_);
		    self.Gradient(g.data());
		    return vec(g);
	    });

	py::class_<TreeModelInterface, ModelInterface>(m, "TreeModelInterface")
	    .def("get_node_count", &TreeModelInterface::GetNodeCount)
	    .def("get_tip_count", &TreeModelInterface::GetTipCount)
	    .def_readonly("node_map", &TreeModelInterface::nodeMap_)
	    .def("describe", [](TreeModelInterface &self) {  // node table, for checking the id conventions against fixtures
		    const phyamd::Tree &t = *self.GetTree();
		    py::dict d;
		    d["left"] = t.left;
		    d["right"] = t.right;
		    d["parent"] = t.parent;
		    d["class_id"] = t.class_id;
		    d["name"] = t.name;
		    d["distance"] = t.distance;
		    d["height"] = t.height;
		    d["root"] = t.root;
		    d["lowers"] = t.lowers;
		    d["ratios"] = t.ratios;
		    d["postorder"] = t.postorder;
		    return d;
	    });
	py::class_<UnRootedTreeModelInterface, TreeModelInterface>(m, "UnRootedTreeModelInterface")
	    .def(py::init<const std::string &, const std::vector<std::string> &>());
	py::class_<TimeTreeModelInterface, TreeModelInterface>(m, "TimeTreeModelInterface")
	    .def(py::init<const std::string &, const std::vector<std::string> &, const std::vector<double>>())
	    .def("get_node_heights", [](TimeTreeModelInterface &self) {
		    std::vector<double> h(self.GetTipCount() - 1);
		    self.GetNodeHeights(h.data());
		    return vec(h);
	    });
	py::class_<ReparameterizedTimeTreeModelInterface, TimeTreeModelInterface>(m, "ReparameterizedTimeTreeModelInterface")
	    .def(py::init<const std::string &, const std::vector<std::string> &, const std::vector<double>, TreeTransformFlags>())
	    .def("gradient_transform_jvp",
	         [](ReparameterizedTimeTreeModelInterface &self, darray hg) {
		         std::vector<double> g(self.GetTipCount() - 1);
		         self.GradientTransformJVP(g.data(), hg.data());
		         return vec(g);
	         })
	    .def("gradient_transform_jvp_with_heights",
	         [](ReparameterizedTimeTreeModelInterface &self, darray hg, darray heights) {
		         std::vector<double> g(self.GetTipCount() - 1);
		         self.GradientTransformJVP(g.data(), hg.data(), heights.data());
		         return vec(g);
	         })
	    .def("gradient_transform_jacobian",
	         [](ReparameterizedTimeTreeModelInterface &self) {
		         std::vector<double> g(self.GetTipCount() - 1);
		         self.GradientTransformJacobian(g.data());
		         return vec(g);
	         })
	    .def("transform_jacobian", &ReparameterizedTimeTreeModelInterface::TransformJacobian);

	py::class_<BranchModelInterface, ModelInterface>(m, "BranchModelInterface").def("set_rates", [](BranchModelInterface &self, darray r) {
		self.SetRates(r.data());
	});
	py::class_<StrictClockModelInterface, BranchModelInterface>(m, "StrictClockModelInterface")
	    .def(py::init<double, TreeModelInterface *>(), py::keep_alive<1, 3>())
	    .def("set_rate", &StrictClockModelInterface::SetRate);
	py::class_<SimpleClockModelInterface, BranchModelInterface>(m, "SimpleClockModelInterface")
	    .def(py::init<const std::vector<double> &, TreeModelInterface *>(), py::keep_alive<1, 3>());

	py::class_<SubstitutionModelInterface, ModelInterface>(m, "SubstitutionModelInterface")
	    .def("transition_matrix",  // host-side P(t) / dP/dt of the current parameters: parity checks of the eigen system
	         [](SubstitutionModelInterface &self, double t, bool derivative) {
		         phyamd::SubstModel &sm = *self.GetModel();
		         std::vector<double> P((size_t)sm.S * sm.S);
		         sm.p_t(t, P.data(), derivative);
		         return darray({sm.S, sm.S}, P.data());
	         },
	         py::arg("t"), py::arg("derivative") = false)
	    .def("rate_matrix_derivatives",  // dQ/dtheta [count][S][S] as uploaded for the substitution-model gradient
	         [](SubstitutionModelInterface &self, bool rates, bool frequencies) {
		         phyamd::SubstModel &sm = *self.GetModel();
		         std::vector<double> dQ;
		         sm.rate_matrix_derivatives(rates, frequencies, dQ);
		         return darray({(py::ssize_t)(dQ.size() / ((size_t)sm.S * sm.S)), (py::ssize_t)sm.S, (py::ssize_t)sm.S}, dQ.data());
	         },
	         py::arg("rates") = true, py::arg("frequencies") = true)
	    .def("eigen_system", [](SubstitutionModelInterface &self) {
		    phyamd::SubstModel &sm = *self.GetModel();
		    sm.update();
		    return py::make_tuple(vec(sm.eval), darray({sm.S, sm.S}, sm.evec.data()), darray({sm.S, sm.S}, sm.ivec.data()),
		                          darray({sm.S, sm.S}, sm.Q.data()));
	    });
	py::class_<JC69Interface, SubstitutionModelInterface>(m, "JC69Interface").def(py::init<>());
	py::class_<HKYInterface, SubstitutionModelInterface>(m, "HKYInterface")
	    .def(py::init<double, const std::vector<double> &>())
	    .def("set_kappa", &HKYInterface::SetKappa)
	    .def("set_frequencies", [](HKYInterface &self, darray f) { self.SetFrequencies(f.data()); });
	py::class_<GTRInterface, SubstitutionModelInterface>(m, "GTRInterface")
	    .def(py::init<const std::vector<double> &, const std::vector<double> &>())
	    .def("set_rates", [](GTRInterface &self, darray r) { self.SetRates(r.data()); })
	    .def("set_frequencies", [](GTRInterface &self, darray f) { self.SetFrequencies(f.data()); });
	py::class_<GeneralSubstitutionModelInterface, SubstitutionModelInterface>(m, "GeneralSubstitutionModelInterface")
	    .def(py::init<DataTypeInterface *, const std::vector<double> &, const std::vector<double> &, const std::vector<unsigned> &, bool>(),
	         py::keep_alive<1, 2>())
	    .def("set_rates", [](GeneralSubstitutionModelInterface &self, darray r) { self.SetRates(r.data()); })
	    .def("set_frequencies", [](GeneralSubstitutionModelInterface &self, darray f) { self.SetFrequencies(f.data()); });

	py::class_<SiteModelInterface, ModelInterface>(m, "SiteModelInterface")
	    .def("set_mu", &SiteModelInterface::SetMu)
	    .def("rates", [](SiteModelInterface &self) {
		    self.GetModel()->update();
		    std::vector<double> r(self.GetModel()->cat_count);
		    self.GetRates(r.data());
		    return vec(r);
	    })
	    .def("proportions", [](SiteModelInterface &self) {
		    self.GetModel()->update();
		    std::vector<double> r(self.GetModel()->cat_count);
		    self.GetProportions(r.data());
		    return vec(r);
	    });
	py::class_<ConstantSiteModelInterface, SiteModelInterface>(m, "ConstantSiteModelInterface")
	    .def(py::init<std::optional<double>>(), py::arg("mu") = py::none());
	py::class_<InvariantSiteModelInterface, SiteModelInterface>(m, "InvariantSiteModelInterface")
	    .def(py::init<double, std::optional<double>>(), py::arg("proportion_invariant"), py::arg("mu") = py::none())
	    .def("set_proportion_invariant", &InvariantSiteModelInterface::SetProportionInvariant);
	py::class_<DiscretizedSiteModelInterface, SiteModelInterface>(m, "DiscretizedSiteModelInterface")
	    .def("set_parameter", &DiscretizedSiteModelInterface::SetParameter)
	    .def("set_proportion_invariant", &DiscretizedSiteModelInterface::SetProportionInvariant)
	    .def("get_category_count", &DiscretizedSiteModelInterface::GetCategoryCount);
	py::class_<WeibullSiteModelInterface, DiscretizedSiteModelInterface>(m, "WeibullSiteModelInterface")
	    .def(py::init<double, size_t, std::optional<double>, std::optional<double>>(), py::arg("shape"), py::arg("categories"),
	         py::arg("proportion_invariant") = py::none(), py::arg("mu") = py::none())
	    .def("set_shape", &WeibullSiteModelInterface::SetShape);
	py::class_<GammaSiteModelInterface, DiscretizedSiteModelInterface>(m, "GammaSiteModelInterface")
	    .def(py::init<double, size_t, std::optional<double>, std::optional<double>>(), py::arg("shape"), py::arg("categories"),
	         py::arg("proportion_invariant") = py::none(), py::arg("mu") = py::none())
	    .def("set_shape", &GammaSiteModelInterface::SetShape)
	    .def("set_epsilon", &GammaSiteModelInterface::SetEpsilon);

	py::class_<TreeLikelihoodInterface, CallableModelInterface>(m, "TreeLikelihoodInterface")
	    .def(py::init<const std::vector<std::pair<std::string, std::string>> &, TreeModelInterface *, SubstitutionModelInterface *,
	                  SiteModelInterface *, std::optional<BranchModelInterface *>, bool, bool, bool>(),
	         py::arg("alignment"), py::arg("tree_model"), py::arg("substitution_model"), py::arg("site_model"), py::arg("branch_model") = py::none(),
	         py::arg("use_ambiguities") = false, py::arg("use_tip_states") = false, py::arg("include_jacobian") = false, py::keep_alive<1, 3>(),
	         py::keep_alive<1, 4>(), py::keep_alive<1, 5>(), py::keep_alive<1, 6>())
	    .def(py::init<const std::vector<std::string> &, const std::vector<std::string> &, TreeModelInterface *, SubstitutionModelInterface *,
	                  SiteModelInterface *, std::optional<BranchModelInterface *>, bool, bool, bool>(),
	         py::arg("taxa"), py::arg("attributes"), py::arg("tree_model"), py::arg("substitution_model"), py::arg("site_model"),
	         py::arg("branch_model") = py::none(), py::arg("use_ambiguities") = false, py::arg("use_tip_states") = false,
	         py::arg("include_jacobian") = false, py::keep_alive<1, 4>(), py::keep_alive<1, 5>(), py::keep_alive<1, 6>(), py::keep_alive<1, 7>())
	    .def("request_gradient", &TreeLikelihoodInterface::RequestGradient, py::arg("flags") = std::vector<TreeLikelihoodGradientFlags>())
	    .def("set_reference_compatibility", &TreeLikelihoodInterface::SetReferenceCompatibility)
	    .def("log_likelihood_batch", [](TreeLikelihoodInterface &self, darray params) {
		    if (params.ndim() != 2 || (size_t)params.shape(1) != self.TreeParameterCount()) throw phyamd::Error("tree parameters: [count][parameter_count]");
		    std::vector<double> lnl((size_t)params.shape(0));
		    self.LogLikelihoodBatch(lnl.size(), params.data(), lnl.data());
		    return vec(lnl);
	    })
	    .def("gradient_batch", [](TreeLikelihoodInterface &self, darray params) {
		    if (params.ndim() != 2 || (size_t)params.shape(1) != self.TreeParameterCount()) throw phyamd::Error("tree parameters: [count][parameter_count]");
		    const size_t count = (size_t)params.shape(0);
		    std::vector<double> lnl(count), g(count * self.gradientLength_);
		    self.GradientBatch(count, params.data(), lnl.data(), g.data());
		    return py::make_tuple(vec(lnl), darray({(py::ssize_t)count, (py::ssize_t)self.gradientLength_}, g.data()));
	    })
	    .def("gradient_weights", [](TreeLikelihoodInterface &self, darray weights, std::optional<darray> params) {
		    if (weights.ndim() != 2 || (size_t)weights.shape(1) != self.GetPatternCount()) throw phyamd::Error("weights: [count][pattern_count]");
		    const size_t count = (size_t)weights.shape(0);
		    if (params && (params->ndim() != 2 || (size_t)params->shape(0) != count || (size_t)params->shape(1) != self.TreeParameterCount()))
			    throw phyamd::Error("tree parameters: [count][parameter_count]");
		    std::vector<double> lnl(count), g(count * self.gradientLength_);
		    self.GradientWeights(count, weights.data(), params ? params->data() : nullptr, lnl.data(), g.data());
		    return py::make_tuple(vec(lnl), darray({(py::ssize_t)count, (py::ssize_t)self.gradientLength_}, g.data()));
	    }, py::arg("weights"), py::arg("tree_parameters") = py::none())
	    .def("log_likelihood_trees", [](TreeLikelihoodInterface &self, iarray left, iarray right, iarray roots, darray lengths) {
		    const size_t count = check_trees(self, left, right, roots, lengths);
		    std::vector<double> lnl(count);
		    self.LogLikelihoodTrees(count, left.data(), right.data(), roots.data(), lengths.data(), lnl.data());
		    return vec(lnl);
	    })
	    .def("gradient_trees", [](TreeLikelihoodInterface &self, iarray left, iarray right, iarray roots, darray lengths) {
		    const size_t count = check_trees(self, left, right, roots, lengths), N = self.NodeCount();
		    std::vector<double> lnl(count), g(count * N);
		    self.GradientTrees(count, left.data(), right.data(), roots.data(), lengths.data(), lnl.data(), g.data());
		    return py::make_tuple(vec(lnl), darray({(py::ssize_t)count, (py::ssize_t)N}, g.data()));
	    })
	    .def("pattern_log_likelihoods_trees", [](TreeLikelihoodInterface &self, iarray left, iarray right, iarray roots, darray lengths, std::optional<darray> weights,
	                                             bool want_patterns) -> py::tuple {
		    const size_t count = check_trees(self, left, right, roots, lengths);
		    const py::ssize_t P = (py::ssize_t)self.GetPatternCount();
		    if (weights && (weights->ndim() != 2 || weights->shape(0) < 1 || weights->shape(1) != P)) throw phyamd::Error("replicate weights: [replicates >= 1][patterns]");
		    const size_t R = weights ? (size_t)weights->shape(0) : 0;
		    std::vector<double> lnl(count), rows(want_patterns ? count * (size_t)P : 0), rep(R * count);
		    self.PatternLogLikelihoodsTrees(count, left.data(), right.data(), roots.data(), lengths.data(), lnl.data(), want_patterns ? rows.data() : nullptr, R,
		                                    weights ? weights->data() : nullptr, R ? rep.data() : nullptr);
		    py::object rows_out = py::none(), rep_out = py::none();
		    if (want_patterns) rows_out = darray({(py::ssize_t)count, P}, rows.data());
		    if (R) rep_out = darray({(py::ssize_t)R, (py::ssize_t)count}, rep.data());
		    return py::make_tuple(vec(lnl), rows_out, rep_out);
	    }, py::arg("left"), py::arg("right"), py::arg("roots"), py::arg("branch_lengths"), py::arg("replicate_weights") = py::none(), py::arg("want_patterns") = true)
	    .def("nni_log_likelihoods", [](TreeLikelihoodInterface &self, std::optional<darray> central, bool want_derivatives) -> py::tuple {
		    const py::ssize_t N = (py::ssize_t)self.NodeCount();
		    if (central && (central->ndim() != 2 || central->shape(0) != 3 || central->shape(1) != N)) throw phyamd::Error("central lengths: [3][node_count]");
		    std::vector<double> lnl((size_t)3 * N), d1(want_derivatives ? lnl.size() : 0), d2(d1.size());
		    self.NNILogLikelihoods(central ? central->data() : nullptr, lnl.data(), want_derivatives ? d1.data() : nullptr, want_derivatives ? d2.data() : nullptr);
		    const std::vector<py::ssize_t> shape{3, N};
		    if (!want_derivatives) return py::make_tuple(darray(shape, lnl.data()), py::none(), py::none());
		    return py::make_tuple(darray(shape, lnl.data()), darray(shape, d1.data()), darray(shape, d2.data()));
	    }, py::arg("central_lengths") = py::none(), py::arg("want_derivatives") = true)
	    .def("nni_log_likelihoods_general", [](TreeLikelihoodInterface &self, std::optional<darray> central, bool want_derivatives) -> py::tuple {
		    const py::ssize_t N = (py::ssize_t)self.NodeCount();
		    if (central && (central->ndim() != 2 || central->shape(0) != 3 || central->shape(1) != N)) throw phyamd::Error("central lengths: [3][node_count]");
		    std::vector<double> lnl((size_t)3 * N), d1(want_derivatives ? lnl.size() : 0), d2(d1.size());
		    self.NNILogLikelihoodsGeneral(central ? central->data() : nullptr, lnl.data(), want_derivatives ? d1.data() : nullptr, want_derivatives ? d2.data() : nullptr);
		    const std::vector<py::ssize_t> shape{3, N};
		    if (!want_derivatives) return py::make_tuple(darray(shape, lnl.data()), py::none(), py::none());
		    return py::make_tuple(darray(shape, lnl.data()), darray(shape, d1.data()), darray(shape, d2.data()));
	    }, py::arg("central_lengths") = py::none(), py::arg("want_derivatives") = true)
	    .def("nni_optimize", [](TreeLikelihoodInterface &self, std::optional<darray> start, double lower, double upper, double tolerance, int max_iterations) -> py::tuple {
		    const py::ssize_t N = (py::ssize_t)self.NodeCount();
		    if (start && (start->ndim() != 2 || start->shape(0) != 3 || start->shape(1) != N)) throw phyamd::Error("start lengths: [3][node_count]");
		    std::vector<double> len((size_t)3 * N), lnl(len.size()), d1(len.size()), d2(len.size());
		    std::vector<int32_t> it(len.size());
		    self.NNIOptimize(start ? start->data() : nullptr, lower, upper, tolerance, max_iterations, len.data(), lnl.data(), d1.data(), d2.data(), it.data());
		    const std::vector<py::ssize_t> shape{3, N};
		    return py::make_tuple(darray(shape, len.data()), darray(shape, lnl.data()), darray(shape, d1.data()), darray(shape, d2.data()), iarray(shape, it.data()));
	    }, py::arg("start_lengths") = py::none(), py::arg("lower") = 1e-8, py::arg("upper") = 10.0, py::arg("tolerance") = 1e-8, py::arg("max_iterations") = 100)
	    .def("nni_optimize_general", [](TreeLikelihoodInterface &self, std::optional<darray> start, double lower, double upper, double tolerance, int max_iterations) -> py::tuple {
		    const py::ssize_t N = (py::ssize_t)self.NodeCount();
		    if (start && (start->ndim() != 2 || start->shape(0) != 3 || start->shape(1) != N)) throw phyamd::Error("start lengths: [3][node_count]");
		    std::vector<double> len((size_t)3 * N), lnl(len.size()), d1(len.size()), d2(len.size());
		    std::vector<int32_t> it(len.size());
		    self.NNIOptimizeGeneral(start ? start->data() : nullptr, lower, upper, tolerance, max_iterations, len.data(), lnl.data(), d1.data(), d2.data(), it.data());
		    const std::vector<py::ssize_t> shape{3, N};
		    return py::make_tuple(darray(shape, len.data()), darray(shape, lnl.data()), darray(shape, d1.data()), darray(shape, d2.data()), iarray(shape, it.data()));
	    }, py::arg("start_lengths") = py::none(), py::arg("lower") = 1e-8, py::arg("upper") = 10.0, py::arg("tolerance") = 1e-8, py::arg("max_iterations") = 100)
	    .def("optimize_branch_lengths", [](TreeLikelihoodInterface &self, iarray left, iarray right, iarray roots, darray lengths, std::optional<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>> optimise,
	                                       double lower, double upper, double tolerance, int max_iterations, double lnl_tolerance, int max_passes) -> py::tuple {
		    const size_t count = check_trees(self, left, right, roots, lengths);
		    const py::ssize_t N = (py::ssize_t)self.NodeCount();
		    if (optimise && (optimise->ndim() != 2 || (size_t)optimise->shape(0) != count || optimise->shape(1) != N)) throw phyamd::Error("optimise: [count][node_count]");
		    std::vector<double> len(count * (size_t)N), lnl(count), lnl0(count);
		    std::vector<int32_t> passes(count);
		    self.OptimizeBranchLengths(count, left.data(), right.data(), roots.data(), lengths.data(), optimise ? optimise->data() : nullptr, lower, upper, tolerance,
		                               max_iterations, lnl_tolerance, max_passes, len.data(), lnl.data(), lnl0.data(), passes.data());
		    return py::make_tuple(darray({(py::ssize_t)count, N}, len.data()), vec(lnl), vec(lnl0), iarray(std::vector<py::ssize_t>{(py::ssize_t)count}, passes.data()));
	    }, py::arg("left"), py::arg("right"), py::arg("roots"), py::arg("branch_lengths"), py::arg("optimise") = py::none(), py::arg("lower") = 1e-8, py::arg("upper") = 10.0,
	       py::arg("tolerance") = 1e-8, py::arg("max_iterations") = 100, py::arg("lnl_tolerance") = 1e-6, py::arg("max_passes") = 50)
	    .def("spr_log_likelihoods", [](TreeLikelihoodInterface &self, std::optional<iarray> prune) {
		    const py::ssize_t N = (py::ssize_t)self.NodeCount();
		    if (prune && prune->ndim() != 1) throw phyamd::Error("prune: [count]");
		    const py::ssize_t count = prune ? prune->shape(0) : N;
		    std::vector<double> lnl((size_t)count * N);
		    self.SPRLogLikelihoods(prune ? prune->data() : nullptr, (int)count, lnl.data());
		    return darray({count, N}, lnl.data());
	    }, py::arg("prune") = py::none())
	    .def("spr_log_likelihoods_general", [](TreeLikelihoodInterface &self, std::optional<iarray> prune) {
		    const py::ssize_t N = (py::ssize_t)self.NodeCount();
		    if (prune && prune->ndim() != 1) throw phyamd::Error("prune: [count]");
		    const py::ssize_t count = prune ? prune->shape(0) : N;
		    std::vector<double> lnl((size_t)count * N);
		    self.SPRLogLikelihoodsGeneral(prune ? prune->data() : nullptr, (int)count, lnl.data());
		    return darray({count, N}, lnl.data());
	    }, py::arg("prune") = py::none())
	    .def("spr_optimize", [](TreeLikelihoodInterface &self, std::optional<iarray> prune, double lower, double upper, double tolerance, int max_iterations,
	                            double lnl_tolerance, int max_passes) -> py::tuple {
		    const py::ssize_t N = (py::ssize_t)self.NodeCount();
		    if (prune && prune->ndim() != 1) throw phyamd::Error("prune: [count]");
		    const py::ssize_t count = prune ? prune->shape(0) : N;
		    std::vector<double> len((size_t)count * N * 3), lnl((size_t)count * N), lnl0(lnl.size());
		    std::vector<int32_t> passes(lnl.size());
		    self.SPROptimize(prune ? prune->data() : nullptr, (int)count, lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes, len.data(), lnl.data(),
		                     lnl0.data(), passes.data());
		    const std::vector<py::ssize_t> shape{count, N};
		    return py::make_tuple(darray({count, N, (py::ssize_t)3}, len.data()), darray(shape, lnl.data()), darray(shape, lnl0.data()), iarray(shape, passes.data()));
	    }, py::arg("prune") = py::none(), py::arg("lower") = 1e-8, py::arg("upper") = 10.0, py::arg("tolerance") = 1e-8, py::arg("max_iterations") = 100,
	       py::arg("lnl_tolerance") = 1e-6, py::arg("max_passes") = 50)
	    .def("spr_optimize_general", [](TreeLikelihoodInterface &self, std::optional<iarray> prune, double lower, double upper, double tolerance, int max_iterations,
	                                    double lnl_tolerance, int max_passes) -> py::tuple {
		    const py::ssize_t N = (py::ssize_t)self.NodeCount();
		    if (prune && prune->ndim() != 1) throw phyamd::Error("prune: [count]");
		    const py::ssize_t count = prune ? prune->shape(0) : N;
		    std::vector<double> len((size_t)count * N * 3), lnl((size_t)count * N), lnl0(lnl.size());
		    std::vector<int32_t> passes(lnl.size());
		    self.SPROptimizeGeneral(prune ? prune->data() : nullptr, (int)count, lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes, len.data(), lnl.data(),
		                            lnl0.data(), passes.data());
		    const std::vector<py::ssize_t> shape{count, N};
		    return py::make_tuple(darray({count, N, (py::ssize_t)3}, len.data()), darray(shape, lnl.data()), darray(shape, lnl0.data()), iarray(shape, passes.data()));
	    }, py::arg("prune") = py::none(), py::arg("lower") = 1e-8, py::arg("upper") = 10.0, py::arg("tolerance") = 1e-8, py::arg("max_iterations") = 100,
	       py::arg("lnl_tolerance") = 1e-6, py::arg("max_passes") = 50)
	    .def("pairwise_distances", [](TreeLikelihoodInterface &self, std::optional<iarray> pairs, std::optional<darray> start, double lower, double upper, double tolerance,
	                                  int max_iterations, bool want_counts, bool counts_only) -> py::tuple {
		    const py::ssize_t T = ((py::ssize_t)self.NodeCount() + 1) / 2;
		    if (pairs && (pairs->ndim() != 2 || pairs->shape(1) != 2)) throw phyamd::Error("pairs: [count][2]");
		    const py::ssize_t count = pairs ? pairs->shape(0) : T * (T - 1) / 2;
		    if (start && (start->ndim() != 1 || start->shape(0) != count)) throw phyamd::Error("start: [count]");
		    const size_t n = counts_only ? 0 : (size_t)count;
		    std::vector<double> dist(n), lnl(n), d1(n), d2(n), table(want_counts || counts_only ? (size_t)count * 256 : 0);
		    std::vector<int32_t> it(n);
		    self.PairwiseDistances(pairs ? pairs->data() : nullptr, (int)count, start ? start->data() : nullptr, lower, upper, tolerance, max_iterations,
		                           n ? dist.data() : nullptr, n ? lnl.data() : nullptr, n ? d1.data() : nullptr, n ? d2.data() : nullptr, n ? it.data() : nullptr,
		                           table.empty() ? nullptr : table.data());
		    const std::vector<py::ssize_t> shape{count};
		    const auto vec = [&](const std::vector<double> &v) -> py::object { return n ? py::object(darray(shape, v.data())) : py::object(py::none()); };
		    return py::make_tuple(vec(dist), vec(lnl), vec(d1), vec(d2), n ? py::object(iarray(shape, it.data())) : py::object(py::none()),
		                          table.empty() ? py::object(py::none()) : py::object(darray({count, (py::ssize_t)16, (py::ssize_t)16}, table.data())));
	    }, py::arg("pairs") = py::none(), py::arg("start") = py::none(), py::arg("lower") = 1e-8, py::arg("upper") = 10.0, py::arg("tolerance") = 1e-8,
	       py::arg("max_iterations") = 100, py::arg("want_counts") = false, py::arg("counts_only") = false)
	    .def("pairwise_distances_general", [](TreeLikelihoodInterface &self, std::optional<iarray> pairs, std::optional<darray> start, double lower, double upper,
	                                          double tolerance, int max_iterations, bool want_counts, bool counts_only, bool want_class_members) -> py::tuple {
		    const py::ssize_t T = ((py::ssize_t)self.NodeCount() + 1) / 2;
		    if (pairs && (pairs->ndim() != 2 || pairs->shape(1) != 2)) throw phyamd::Error("pairs: [count][2]");
		    const py::ssize_t count = pairs ? pairs->shape(0) : T * (T - 1) / 2;
		    if (start && (start->ndim() != 1 || start->shape(0) != count)) throw phyamd::Error("start: [count]");
		    const size_t n = counts_only ? 0 : (size_t)count;
		    std::vector<double> dist(n), lnl(n), d1(n), d2(n), table(want_counts || counts_only ? (size_t)count * 1024 : 0);
		    std::vector<int32_t> it(n);
		    std::vector<uint64_t> members(want_class_members ? 32 : 0);
		    self.PairwiseDistancesGeneral(pairs ? pairs->data() : nullptr, (int)count, start ? start->data() : nullptr, lower, upper, tolerance, max_iterations,
		                                  n ? dist.data() : nullptr, n ? lnl.data() : nullptr, n ? d1.data() : nullptr, n ? d2.data() : nullptr, n ? it.data() : nullptr,
		                                  table.empty() ? nullptr : table.data(), members.empty() ? nullptr : members.data());
		    const std::vector<py::ssize_t> shape{count};
		    const auto vec = [&](const std::vector<double> &v) -> py::object { return n ? py::object(darray(shape, v.data())) : py::object(py::none()); };
		    return py::make_tuple(vec(dist), vec(lnl), vec(d1), vec(d2), n ? py::object(iarray(shape, it.data())) : py::object(py::none()),
		                          table.empty() ? py::object(py::none()) : py::object(darray({count, (py::ssize_t)32, (py::ssize_t)32}, table.data())),
		                          members.empty() ? py::object(py::none()) : py::object(py::array_t<uint64_t>({(py::ssize_t)32}, members.data())));
	    }, py::arg("pairs") = py::none(), py::arg("start") = py::none(), py::arg("lower") = 1e-8, py::arg("upper") = 10.0, py::arg("tolerance") = 1e-8,
	       py::arg("max_iterations") = 100, py::arg("want_counts") = false, py::arg("counts_only") = false, py::arg("want_class_members") = false)
	    .def("placement_log_likelihoods", [](TreeLikelihoodInterface &self, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> masks, darray pendant, double split,
	                                         bool want_lnl, bool want_best) -> py::tuple {
		    const py::ssize_t N = (py::ssize_t)self.NodeCount();
		    if (masks.ndim() != 2 || (size_t)masks.shape(1) != self.GetPatternCount()) throw phyamd::Error("masks: [queries][pattern_count]");
		    if (pendant.ndim() != 1) throw phyamd::Error("pendant: [lengths]");
		    const py::ssize_t Q = masks.shape(0), L = pendant.shape(0);
		    std::vector<double> lnl(want_lnl ? (size_t)L * Q * N : 0), best(want_best ? (size_t)L * Q : 0);
		    std::vector<int32_t> node(best.size());
		    self.PlacementLogLikelihoods(masks.data(), (int)Q, pendant.data(), (int)L, split, want_lnl ? lnl.data() : nullptr, want_best ? node.data() : nullptr,
		                                 want_best ? best.data() : nullptr);
		    const std::vector<py::ssize_t> shape{L, Q};
		    return py::make_tuple(want_lnl ? py::object(darray({L, Q, N}, lnl.data())) : py::object(py::none()),
		                          want_best ? py::object(iarray(shape, node.data())) : py::object(py::none()),
		                          want_best ? py::object(darray(shape, best.data())) : py::object(py::none()));
	    }, py::arg("masks"), py::arg("pendant"), py::arg("split") = 0.5, py::arg("want_lnl") = true, py::arg("want_best") = true)
	    .def("placement_log_likelihoods_general", [](TreeLikelihoodInterface &self, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> codes, darray pendant,
	                                                 double split, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> sets, bool want_lnl,
	                                                 bool want_best) -> py::tuple {
		    const py::ssize_t N = (py::ssize_t)self.NodeCount();
		    if (codes.ndim() != 2 || (size_t)codes.shape(1) != self.GetPatternCount()) throw phyamd::Error("codes: [queries][pattern_count]");
		    if (pendant.ndim() != 1) throw phyamd::Error("pendant: [lengths]");
		    if (sets.ndim() != 1) throw phyamd::Error("sets: [set_count]");
		    const py::ssize_t Q = codes.shape(0), L = pendant.shape(0), nsets = sets.shape(0);
		    std::vector<double> lnl(want_lnl ? (size_t)L * Q * N : 0), best(want_best ? (size_t)L * Q : 0);
		    std::vector<int32_t> node(best.size());
		    self.PlacementLogLikelihoodsGeneral(codes.data(), (int)Q, nsets ? sets.data() : nullptr, (int)nsets, pendant.data(), (int)L, split, want_lnl ? lnl.data() : nullptr,
		                                        want_best ? node.data() : nullptr, want_best ? best.data() : nullptr);
		    const std::vector<py::ssize_t> shape{L, Q};
		    return py::make_tuple(want_lnl ? py::object(darray({L, Q, N}, lnl.data())) : py::object(py::none()),
		                          want_best ? py::object(iarray(shape, node.data())) : py::object(py::none()),
		                          want_best ? py::object(darray(shape, best.data())) : py::object(py::none()));
	    }, py::arg("codes"), py::arg("pendant"), py::arg("split") = 0.5, py::arg("sets") = py::array_t<uint64_t>(0), py::arg("want_lnl") = true, py::arg("want_best") = true)
	    .def("placement_optimize", [](TreeLikelihoodInterface &self, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> masks, iarray candidates,
	                                  std::optional<darray> pendant_start, double split, int branches, double lower, double upper, double tolerance, int max_iterations,
	                                  double lnl_tolerance, int max_passes) -> py::tuple {
		    if (masks.ndim() != 2 || (size_t)masks.shape(1) != self.GetPatternCount()) throw phyamd::Error("masks: [queries][pattern_count]");
		    if (candidates.ndim() != 2 || candidates.shape(1) != 2) throw phyamd::Error("candidates: [count][2]");
		    const py::ssize_t Q = masks.shape(0), count = candidates.shape(0);
		    if (pendant_start && (pendant_start->ndim() != 1 || pendant_start->shape(0) != count)) throw phyamd::Error("pendant_start: [count]");
		    std::vector<double> len((size_t)count * 3), lnl((size_t)count), lnl0(lnl.size());
		    std::vector<int32_t> passes(lnl.size());
		    self.PlacementOptimize(masks.data(), (int)Q, candidates.data(), (int)count, pendant_start ? pendant_start->data() : nullptr, split, branches, lower, upper, tolerance,
		                           max_iterations, lnl_tolerance, max_passes, len.data(), lnl.data(), lnl0.data(), passes.data());
		    const std::vector<py::ssize_t> shape{count};
		    return py::make_tuple(darray({count, (py::ssize_t)3}, len.data()), darray(shape, lnl.data()), darray(shape, lnl0.data()), iarray(shape, passes.data()));
	    }, py::arg("masks"), py::arg("candidates"), py::arg("pendant_start") = py::none(), py::arg("split") = 0.5, py::arg("branches") = 7, py::arg("lower") = 1e-8,
	       py::arg("upper") = 10.0, py::arg("tolerance") = 1e-8, py::arg("max_iterations") = 100, py::arg("lnl_tolerance") = 1e-6, py::arg("max_passes") = 50)
	    .def("placement_optimize_general", [](TreeLikelihoodInterface &self, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> codes, iarray candidates,
	                                          py::array_t<uint64_t, py::array::c_style | py::array::forcecast> sets, std::optional<darray> pendant_start, double split,
	                                          int branches, double lower, double upper, double tolerance, int max_iterations, double lnl_tolerance,
	                                          int max_passes) -> py::tuple {
		    if (codes.ndim() != 2 || (size_t)codes.shape(1) != self.GetPatternCount()) throw phyamd::Error("codes: [queries][pattern_count]");
		    if (candidates.ndim() != 2 || candidates.shape(1) != 2) throw phyamd::Error("candidates: [count][2]");
		    if (sets.ndim() != 1) throw phyamd::Error("sets: [set_count]");
		    const py::ssize_t Q = codes.shape(0), count = candidates.shape(0), nsets = sets.shape(0);
		    if (pendant_start && (pendant_start->ndim() != 1 || pendant_start->shape(0) != count)) throw phyamd::Error("pendant_start: [count]");
		    std::vector<double> len((size_t)count * 3), lnl((size_t)count), lnl0(lnl.size());
		    std::vector<int32_t> passes(lnl.size());
		    self.PlacementOptimizeGeneral(codes.data(), (int)Q, nsets ? sets.data() : nullptr, (int)nsets, candidates.data(), (int)count,
		                                  pendant_start ? pendant_start->data() : nullptr, split, branches, lower, upper, tolerance, max_iterations, lnl_tolerance, max_passes,
		                                  len.data(), lnl.data(), lnl0.data(), passes.data());
		    const std::vector<py::ssize_t> shape{count};
		    return py::make_tuple(darray({count, (py::ssize_t)3}, len.data()), darray(shape, lnl.data()), darray(shape, lnl0.data()), iarray(shape, passes.data()));
	    }, py::arg("codes"), py::arg("candidates"), py::arg("sets") = py::array_t<uint64_t>(0), py::arg("pendant_start") = py::none(), py::arg("split") = 0.5,
	       py::arg("branches") = 7, py::arg("lower") = 1e-8, py::arg("upper") = 10.0, py::arg("tolerance") = 1e-8, py::arg("max_iterations") = 100,
	       py::arg("lnl_tolerance") = 1e-6, py::arg("max_passes") = 50)
	    .def("state_posteriors", [](TreeLikelihoodInterface &self, std::optional<iarray> nodes, bool want_posteriors, bool want_states) -> py::tuple {
		    const py::ssize_t N = (py::ssize_t)self.NodeCount(), P = (py::ssize_t)self.GetPatternCount(), S = (py::ssize_t)self.StateCount();
		    if (nodes && nodes->ndim() != 1) throw phyamd::Error("nodes: [count]");
		    const py::ssize_t count = nodes ? nodes->shape(0) : N;
		    std::vector<double> post(want_posteriors ? (size_t)(count * P * S) : 0);
		    std::vector<unsigned char> states(want_states ? (size_t)(count * P) : 0);
		    self.StatePosteriors(nodes ? nodes->data() : nullptr, (int)count, want_posteriors ? post.data() : nullptr, want_states ? states.data() : nullptr);
		    py::object a = py::none(), b = py::none();
		    if (want_posteriors) a = darray({count, P, S}, post.data());
		    if (want_states) b = py::array_t<unsigned char>({count, P}, states.data());
		    return py::make_tuple(a, b);
	    }, py::arg("nodes") = py::none(), py::arg("want_posteriors") = true, py::arg("want_states") = true)
	    .def("branch_hessian", [](TreeLikelihoodInterface &self, bool want_gradient) -> py::tuple {
		    const py::ssize_t N = (py::ssize_t)self.NodeCount();
		    std::vector<double> g(want_gradient ? (size_t)N : 0), H((size_t)(N * N));
		    const double lnl = self.BranchHessian(want_gradient ? g.data() : nullptr, H.data());
		    py::object gradient = py::none();
		    if (want_gradient) gradient = vec(g);
		    return py::make_tuple(lnl, gradient, darray({N, N}, H.data()));
	    }, py::arg("want_gradient") = true)
	    .def("site_rate_posteriors", [](TreeLikelihoodInterface &self) {
		    const py::ssize_t P = (py::ssize_t)self.GetPatternCount(), C = (py::ssize_t)self.CategoryCount();
		    std::vector<double> R((size_t)(P * C)), mean((size_t)P);
		    self.SiteRatePosteriors(R.data(), mean.data());
		    return py::make_tuple(darray({P, C}, R.data()), vec(mean));
	    })
	    .def("get_pattern_count", &TreeLikelihoodInterface::GetPatternCount)
	    .def("pattern_weights", [](TreeLikelihoodInterface &self) { return vec(self.PatternWeights()); })
	    .def("pattern_states", [](TreeLikelihoodInterface &self) {
		    const auto &s = self.PatternStates();
		    const py::ssize_t P = (py::ssize_t)self.GetPatternCount();
		    return py::array_t<unsigned char>({(py::ssize_t)(s.size() / (size_t)P), P}, s.data());
	    });

	// --- host-only helpers (CPU tests of the host logic; no device involved) ---
	m.def("compress_patterns", [](const std::string &datatype, const std::vector<std::string> &names, const std::vector<std::string> &seqs) {
		phyamd::DataType dt;
		if (datatype == "nucleotide") dt.kind = phyamd::DataTypeKind::Nucleotide, dt.state_count = 4;
		else if (datatype == "aa") dt.kind = phyamd::DataTypeKind::AminoAcid, dt.state_count = 20;
		else if (datatype == "codon") dt.kind = phyamd::DataTypeKind::Codon, dt.state_count = 61, dt.symbol_length = 3;
		else throw phyamd::Error("unknown datatype " + datatype);
		phyamd::Patterns p = phyamd::compress_patterns(dt, names, seqs);
		return py::make_tuple(py::array_t<unsigned char>({(py::ssize_t)p.taxon_count, (py::ssize_t)p.pattern_count}, p.states.data()), vec(p.weights));
	});
	m.def("compress_patterns_device", [](const std::string &datatype, const std::vector<std::string> &names, const std::vector<std::string> &seqs) {
		phyamd::DataType dt;
		if (datatype == "nucleotide") dt.kind = phyamd::DataTypeKind::Nucleotide, dt.state_count = 4;
		else if (datatype == "aa") dt.kind = phyamd::DataTypeKind::AminoAcid, dt.state_count = 20;
		else if (datatype == "codon") dt.kind = phyamd::DataTypeKind::Codon, dt.state_count = 61, dt.symbol_length = 3;
		else throw phyamd::Error("unknown datatype " + datatype);
		phyamd::Patterns p = phyamd::compress_patterns_device(dt, names, seqs);
		return py::make_tuple(py::array_t<unsigned char>({(py::ssize_t)p.taxon_count, (py::ssize_t)p.pattern_count}, p.states.data()), vec(p.weights));
	});
	// host substitution models by name (JC69, HKY, GTR, WAG, LG, MG94): normalised Q and its eigen system, as uploaded with
	// phyamd_set_eigen / phyamd_set_frequencies.  frequencies = None: the model's own (WAG) or uniform.
	m.def("substitution_model", [](const std::string &name, const std::vector<double> &rates, std::optional<std::vector<double>> frequencies) {
		phyamd::SubstModel sm;
		sm.name = name;
		sm.S = (name == "WAG" || name == "LG") ? 20 : name == "MG94" ? 61 : 4;
		sm.rates = rates;
		if (frequencies) sm.freqs = *frequencies;
		else if (name == "WAG") sm.freqs.assign(phyamd::wag_frequencies(), phyamd::wag_frequencies() + 20);
		else sm.freqs.assign(sm.S, 1.0 / sm.S);
		sm.update();
		const ssize_t S = sm.S;
		py::dict d;
		d["state_count"] = sm.S;
		d["frequencies"] = vec(sm.freqs);
		d["Q"] = darray({S, S}, sm.Q.data());
		d["eval"] = vec(sm.eval);
		d["evec"] = darray({S, S}, sm.evec.data());
		d["ivec"] = darray({S, S}, sm.ivec.data());
		return d;
	}, py::arg("name"), py::arg("rates") = std::vector<double>(), py::arg("frequencies") = std::nullopt);
	m.def("gamma_quantile", &phyamd::gamma_quantile);
	m.def("reg_lower_gamma", &phyamd::reg_lower_gamma);
}
