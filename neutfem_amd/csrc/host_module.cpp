// host_module.cpp -- pybind11 module `neutfem._neutfem_eigen`: the reference's Python surface
// (src/wrapper.cpp:20-1066) re-exported name for name over the MI355X C ABI (include/neutfem_hip.h).
//
// The class keeps what the reference keeps on the host -- cross-section arrays, flux, tolerances,
// BC map, warm-start flags -- and hands the hot path (BuildMatrices, SolveKeff, SolveCoarse,
// build_diagonal_cache, SolveSubcritical, SolveModes, step_transient, set_void (handed over at BuildMatrices), project_flux, project_power, zoom_resolved, sensitivity_maps, SolveGPT, gpt_sensitivity_maps) to the HIP library.  There is NO CPU fallback:
// without a HIP device those methods raise RuntimeError.  The reflector methods the reference binds are accepted and ignored.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <functional>
#include <iomanip>
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/neutfem_hip.h"

namespace py = pybind11;

// include/NeutFEM.hpp:51-91, include/solvers.hpp:176-190
enum class BCType { DIRICHLET, NEUMANN, MIRROR, ROBIN, PERIODIC };
enum class VerbosityLevel { SILENT = 0, LIGHT = 1, NORMAL = 2, VERBOSE = 3, DEBUG = 4 };
enum class BoundaryID { LEFT_1D = 1, RIGHT_1D = 2, LEFT_2D = 1, RIGHT_2D = 2, TOP_2D = 3, BOTTOM_2D = 4,
                        BACK_3D = 1, FRONT_3D = 2, LEFT_3D = 3, RIGHT_3D = 4, TOP_3D = 5, BOTTOM_3D = 6 };
enum class LinearSolverType { DIRECT_LU, DIRECT_LDLT, DIRECT_LLT, CG, CG_DIAG, CG_ICHOL, BICGSTAB, BICGSTAB_DIAG, BICGSTAB_ILU, LCG };

using arr_t = py::array_t<double, py::array::c_style | py::array::forcecast>;

class NeutFEM {
public:
    NeutFEM(int order, int ng, arr_t xb, arr_t yb, arr_t zb) : NeutFEM(order, order, ng, xb, yb, zb) {}
    NeutFEM(int rt_order, int p_order, int ng, arr_t xb, arr_t yb, arr_t zb)
    {
        if (xb.ndim() != 1 || yb.ndim() != 1 || zb.ndim() != 1) throw std::runtime_error("breaks must be 1-D arrays");
        xb_.assign(xb.data(), xb.data() + xb.size()); yb_.assign(yb.data(), yb.data() + yb.size()); zb_.assign(zb.data(), zb.data() + zb.size());
        if (xb_.size() < 2) throw std::runtime_error("x_breaks needs at least 2 entries");
        nx_ = (int)xb_.size() - 1; ny_ = yb_.size() > 1 ? (int)yb_.size() - 1 : 1; nz_ = zb_.size() > 1 ? (int)zb_.size() - 1 : 1;
        dim_ = nz_ > 1 ? 3 : (ny_ > 1 ? 2 : 1);
        ng_ = ng; rt_ = std::min(rt_order, 2); p_ = std::min(p_order, 2);
        if (rt_ < p_) {                                           // src/NeutFEM.cpp:149-169
            Log(VerbosityLevel::NORMAL, "");
            Log(VerbosityLevel::NORMAL, "!!! ERREUR: RT" + std::to_string(rt_) + "-P" + std::to_string(p_) + " est instable !!!");
            Log(VerbosityLevel::NORMAL, "    Pour la stabilite inf-sup, il faut k_RT >= k_P");
            Log(VerbosityLevel::NORMAL, "    Combinaisons valides: RT0-P0, RT1-P0, RT1-P1, RT2-P0, RT2-P1, RT2-P2");
            Log(VerbosityLevel::NORMAL, "    Forçage à RT" + std::to_string(rt_) + "-P" + std::to_string(rt_));
            Log(VerbosityLevel::NORMAL, "");
            p_ = rt_;
        }
        const int k = rt_, m = p_;                                // src/FEM.cpp:177-259
        nloc_ = dim_ == 1 ? m + 1 : dim_ == 2 ? (m + 1) * (m + 1) : (m + 1) * (m + 1) * (m + 1);
        const int nf = dim_ == 1 ? 1 : dim_ == 2 ? k + 1 : (k + 1) * (k + 1);
        const int ni = dim_ == 1 ? k : dim_ == 2 ? k * (k + 1) : k * (k + 1) * (k + 1);
        ne_ = (long)nx_ * ny_ * nz_; nphi_ = ne_ * nloc_;
        long njx = (long)(nx_ + 1) * ny_ * nz_ * nf, njy = dim_ >= 2 ? (long)nx_ * (ny_ + 1) * nz_ * nf : 0,
             njz = dim_ == 3 ? (long)nx_ * ny_ * (nz_ + 1) * nf : 0;
        nJface_ = njx + njy + njz; nJ_ = nJface_ + ne_ * dim_ * ni;
        D_.assign(ng * ne_, 1.0); SRC_.assign(ng * ne_, 0.0); SigR_.assign(ng * ne_, 0.01); NSF_.assign(ng * ne_, 0.0);
        KSF_.assign(ng * ne_, 0.0); Chi_.assign(ng * ne_, 0.0); SigS_.assign((size_t)ng * ng * ne_, 0.0);
        if (ng > 0) std::fill(Chi_.begin(), Chi_.begin() + ne_, 1.0);
        Phi_.assign(ng * nphi_, 1.0); PhiAdj_.assign(ng * nphi_, 1.0);
        const std::string o = "RT" + std::to_string(rt_) + "-P" + std::to_string(p_);
        Log(VerbosityLevel::NORMAL, "========================================");
        Log(VerbosityLevel::NORMAL, "  NeutFEM - Solveur " + o + " (MI355X / HIP)");
        Log(VerbosityLevel::NORMAL, "========================================");
        Log(VerbosityLevel::NORMAL, "  Dimension     : " + std::to_string(dim_) + "D");
        Log(VerbosityLevel::NORMAL, "  Maillage      : " + std::to_string(nx_) + " x " + std::to_string(ny_) + " x " + std::to_string(nz_));
        Log(VerbosityLevel::NORMAL, "  Elements      : " + std::to_string(ne_));
        Log(VerbosityLevel::NORMAL, "  Groupes       : " + std::to_string(ng));
        Log(VerbosityLevel::NORMAL, "  DOFs flux     : " + std::to_string(nphi_) + " par groupe");
        Log(VerbosityLevel::NORMAL, "  DOFs courant  : " + std::to_string(nJ_) + " par groupe");
        Log(VerbosityLevel::NORMAL, "    - Face DOFs   : " + std::to_string(nJface_));
        Log(VerbosityLevel::NORMAL, "    - Interior DOFs: " + std::to_string(nJ_ - nJface_));
        Log(VerbosityLevel::NORMAL, "========================================\n");
    }
    ~NeutFEM() { if (h_) nf_destroy(h_); }
    NeutFEM(const NeutFEM &) = delete;

    // ---- configuration (src/NeutFEM.cpp:306-362) ------------------------------------------------
    void SetBC(int attr, BCType t, double v) { bc_types_[attr] = t; bc_values_[attr] = v; if (h_ && attr >= 0 && attr < 8) nf_set_bc(h_, attr, (int)t); }
    void SetRobin(int attr, double a, double b) { robin_[attr] = {a, b}; }
    void SetLinearSolver(LinearSolverType t) { solver_ = t; solver_pushed_ = true; }
    void SetTolerance(double tk, double tf, double tl, int mo, int mi) { tol_keff_ = tk; tol_flux_ = tf; tol_L2_ = tl; max_outer_ = mo; max_inner_ = mi; }
    void SetVerbosity(VerbosityLevel v) { verb_ = v; }
    void SetCMFDRelaxation(double w) { cmfd_omega_ = w; if (h_) nf_set_cmfd_relaxation(h_, w); }   // include/NeutFEM.hpp:232-235
    void InitializeCMFD() { need_built("initialize_cmfd"); chk(nf_initialize_cmfd(h_)); }                 // src/NeutFEM.cpp:662-704
    void ApplyQuarterSymmetry(int, int) { SetBC(1, BCType::MIRROR, 0.0); SetBC(4, BCType::MIRROR, 0.0); }   // :356-362
    int AddReflector(py::array_t<double>, py::array_t<double>, py::array_t<double>) { return 0; }           // :2614-2620
    void SetReflector(int, int, bool) {}
    void ClearReflectors() {}
    void ResetFlux()
    {
        std::fill(Phi_.begin(), Phi_.end(), 1.0); std::fill(PhiAdj_.begin(), PhiAdj_.end(), 1.0);
        has_valid_keff_ = false; has_valid_adjoint_ = false;     // src/NeutFEM.cpp:347-354
        if (h_) nf_reset_flux(h_);
    }
    std::string GetSolverName() const
    {
        static const char *n[] = { "SparseLU", "SimplicialLDLT", "SimplicialLLT", "CG", "CG + Diag", "CG + IChol", "BiCGSTAB", "BiCGSTAB + Diag", "BiCGSTAB + ILU", "LSCG" };
        int i = (int)solver_; return i >= 0 && i < 10 ? n[i] : "Unknown";
    }

    // Cut-out cells (extension; include/neutfem_hip.h, nf_set_void): cells with a non-zero mask entry leave the domain and
    // every face a kept cell shares with one carries J.n = gamma phi.  mask is shaped like one group of get_D(), any integer or bool
    // dtype.  Kept on the object and handed to the handle at BuildMatrices(), the way the boundary types are.
    std::vector<py::ssize_t> cell_shape() const
    {
        std::vector<py::ssize_t> shape;
        if (dim_ >= 3) shape.push_back(nz_);
        if (dim_ >= 2) shape.push_back(ny_);
        shape.push_back(nx_);
        return shape;
    }
    void SetVoid(py::array mask, double gamma)
    {
        const std::vector<py::ssize_t> shape = cell_shape();
        bool ok = mask.ndim() == (py::ssize_t)shape.size();
        for (size_t i = 0; ok && i < shape.size(); ++i) ok = mask.shape((py::ssize_t)i) == shape[i];
        if (!ok) throw std::invalid_argument("set_void: the mask must be shaped like one group of get_D()");
        if (!std::isfinite(gamma) || !(gamma > 0.0)) throw std::invalid_argument("set_void: gamma must be finite and positive");
        auto nz = py::array_t<bool, py::array::c_style | py::array::forcecast>::ensure(py::module_::import("numpy").attr("not_equal")(mask, 0));
        if (!nz) throw std::invalid_argument("set_void: the mask must be an integer or bool array");
        std::vector<unsigned char> v((size_t)ne_);
        long cnt = 0;
        for (long e = 0; e < ne_; ++e) { v[e] = nz.data()[e] ? 1 : 0; cnt += v[e]; }
        if (cnt == ne_) throw std::invalid_argument("set_void: every cell is void");
        void_.swap(v); void_gamma_ = gamma;
    }
    void ClearVoid() { void_.clear(); void_gamma_ = 0.0; }
    py::object GetVoid() const
    {
        if (void_.empty()) return py::none();
        py::array_t<bool> m(cell_shape());
        for (long e = 0; e < ne_; ++e) m.mutable_data()[e] = void_[e] != 0;
        return py::make_tuple(m, void_gamma_);
    }

    // ---- hot path ---------------------------------------------------------------------------------
    void BuildMatrices()
    {
        Log(VerbosityLevel::NORMAL, "Assemblage des matrices...");
        ensure_handle();
        for (auto &kv : bc_types_) if (kv.first >= 0 && kv.first < 8) chk(nf_set_bc(h_, kv.first, (int)kv.second));
        if (!void_.empty() || void_on_handle_) { chk(nf_set_void(h_, void_.empty() ? nullptr : void_.data(), void_gamma_)); void_on_handle_ = !void_.empty(); }
        chk(nf_upload_xs(h_, D_.data(), SigR_.data(), NSF_.data(), Chi_.data(), SigS_.data()));
        chk(nf_build(h_));
        Log(VerbosityLevel::NORMAL, "  Assemblage termine (coefficients + factorisation par lignes sur GPU)");
    }
    nf_keff_opts make_opts(bool use_coarse, const std::vector<int> &f, bool use_diag) const
    {
        nf_keff_opts o{}; o.tol_keff = tol_keff_; o.tol_flux = tol_flux_; o.max_outer = max_outer_; o.max_inner = max_inner_;
        o.use_coarse_init = use_coarse && !f.empty();
        o.n_coarse_factors = (int)std::min<size_t>(f.size(), 3);
        for (int i = 0; i < o.n_coarse_factors; ++i) o.coarse_factors[i] = f[i];
        o.use_diagonal_solver = use_diag; o.solver_type = (int)solver_; o.solver_type_pushed = solver_pushed_; o.profile = 0;
        return o;
    }
    int printed_upto_ = 0;                                        // first outer whose progress line has not been printed yet (multiple of 5)
    static void progress_line(void *self, int it, double keff, double dk, double dphi)
    {
        NeutFEM *me = static_cast<NeutFEM *>(self);
        if (it % 5 != 0) return;
        std::cout << "  It " << std::setw(4) << it << " : k = " << std::fixed << std::setprecision(8) << keff << "  dk = " << std::scientific
                  << std::setprecision(2) << dk << "  dphi = " << dphi << std::defaultfloat << std::endl;
        me->printed_upto_ = it + 5;
    }
    // SolveKeff in two halves around the solve itself, which SolveKeffBatch (below the class) shares: the banner, the host mirror and the warm
    // state pushed to the handle, this object's options; then the flux pulled back, the closing lines, last_keff_
    nf_keff_opts keff_prepare(bool use_coarse_init, const std::vector<int> &coarse_factors, bool use_diagonal_solver, bool use_cmfd, const char *who)
    {
        need_built(who);
        Log(VerbosityLevel::NORMAL, "\n=== CALCUL DE K-EFFECTIF (DIRECT) ===");
        if (use_diagonal_solver && !(rt_ == 0 && p_ == 0)) { Log(VerbosityLevel::NORMAL, "  Note: Solveur diagonal non disponible (ordre > 0)"); use_diagonal_solver = false; }
        if (use_diagonal_solver) Log(VerbosityLevel::NORMAL, "  Mode: Solveur diagonal RT0-P0 (faible RAM)");
        Log(VerbosityLevel::NORMAL, use_cmfd ? "  Acceleration: CMFD active" : "  Acceleration: Chebyshev");
        chk(nf_set_phi(h_, Phi_.data()));
        chk(nf_set_warm_state(h_, has_valid_keff_ ? 1 : 0, last_keff_));
        nf_keff_opts o = make_opts(use_coarse_init, coarse_factors, use_diagonal_solver);
        o.use_cmfd = use_cmfd ? 1 : 0;
        chk(nf_set_cmfd_relaxation(h_, cmfd_omega_));
        printed_upto_ = 0;
        return o;
    }
    double keff_accept(double k, int nout)
    {
        chk(nf_get_phi(h_, Phi_.data()));
        if (verb_ >= VerbosityLevel::NORMAL) {
            std::vector<double> hk(nout), hdk(nout), hdp(nout);
            nf_get_history(h_, hk.data(), hdk.data(), hdp.data(), nullptr, nout);
            for (int it = printed_upto_; it < nout; it += 5)
                std::cout << "  It " << std::setw(4) << it << " : k = " << std::fixed << std::setprecision(8) << hk[it] << "  dk = " << std::scientific
                          << std::setprecision(2) << hdk[it] << "  dphi = " << hdp[it] << std::defaultfloat << std::endl;
            if (nout < max_outer_) std::cout << "  Convergence en " << nout << " iterations" << std::endl;
            std::cout << "  k-eff direct = " << std::fixed << std::setprecision(8) << k << std::defaultfloat << std::endl;
        }
        has_valid_keff_ = true; last_keff_ = k;
        return k;
    }
    double SolveKeff(bool use_coarse_init, const std::vector<int> &coarse_factors, bool use_diagonal_solver, bool use_cmfd)
    {
        nf_keff_opts o = keff_prepare(use_coarse_init, coarse_factors, use_diagonal_solver, use_cmfd, "SolveKeff");
        double k = 1.0; int nout = 0;
        // the reference prints its progress line every 5th outer DURING the solve (src/NeutFEM.cpp:1791-1796): the host-driven loop calls back after
        // every outer; the in-kernel paths (milliseconds) have no host in between, their lines follow from the recorded history
        chk(nf_set_progress_callback(h_, verb_ >= VerbosityLevel::NORMAL ? &NeutFEM::progress_line : nullptr, this));
        const int rc_solve = nf_solve_keff(h_, &o, &k, &nout);
        (void)nf_set_progress_callback(h_, nullptr, nullptr);
        chk(rc_solve);
        return keff_accept(k, nout);
    }
    nf_handle handle() const { return h_; }
    void progress_on(bool on) { (void)nf_set_progress_callback(h_, on && verb_ >= VerbosityLevel::NORMAL ? &NeutFEM::progress_line : nullptr, on ? this : nullptr); }
    // SolveSubcritical (include/NeutFEM.hpp:275-279, src/wrapper.cpp:699-715; declared, never defined there): fixed-source solve with the
    // source of get_SRC(), uploaded on every call (a source set after BuildMatrices counts); returns M = flux with / without fission
    double SolveSubcritical()
    {
        need_built("SolveSubcritical");
        Log(VerbosityLevel::NORMAL, "\n=== CALCUL SOUS-CRITIQUE (SOURCE EXTERNE) ===");
        chk(nf_upload_source(h_, SRC_.data()));
        nf_keff_opts o = make_opts(false, {}, false);
        nf_subcrit_result r{};
        chk(nf_solve_subcritical(h_, &o, &r));
        chk(nf_get_phi(h_, Phi_.data()));
        subcrit_ = r; has_subcrit_ = true;
        if (verb_ >= VerbosityLevel::NORMAL) {
            std::cout << "  Sans fission : " << r.n_outer_nofission << " iterations, avec fission : " << r.n_outer << " iterations"
                      << (r.converged ? "" : " (non converge)") << std::endl;
            std::cout << "  Rapport de convergence = " << std::fixed << std::setprecision(6) << r.ratio << "  k-source = " << r.k_source
                      << std::defaultfloat << std::endl;
            std::cout << "  Facteur d'amplification M = " << std::fixed << std::setprecision(8) << r.M << std::defaultfloat << std::endl;
        }
        return r.M;
    }
    py::dict GetSubcriticalInfo() const
    {
        if (!has_subcrit_) throw std::runtime_error("get_subcritical_info: call SolveSubcritical() first");
        const nf_subcrit_result &r = subcrit_;
        py::dict d;
        d["M"] = r.M; d["k_source"] = r.k_source; d["ratio"] = r.ratio; d["phi_int"] = r.phi_int; d["phi_int_nofission"] = r.phi_int_nofission;
        d["production"] = r.production; d["source"] = r.source; d["n_outer"] = r.n_outer; d["n_outer_nofission"] = r.n_outer_nofission;
        d["cg_total"] = r.cg_total; d["converged"] = r.converged;
        return d;
    }
    // Space-time kinetics (extension; include/neutfem_hip.h, nf_transient_*).  begin_transient pushes the host flux mirror and
    // starts from it with keff (default: GetLastKeff()); a perturbation is an edit of a get_SigR() .. view followed by BuildMatrices();
    // step_transient advances n_steps implicit-Euler steps with the tolerances and the linear solver of this object, returns P / P(0) per
    // step and pulls the new flux into the mirror (get_flux(), ExportVTK see time t).  GetLastKeff stays as it is.
    void BeginTransient(arr_t velocity, arr_t beta, arr_t decay, py::object chi_delayed, py::object keff)
    {
        need_built("begin_transient");
        if (velocity.size() != ng_) throw std::runtime_error("begin_transient: velocity needs one entry per group");
        if (beta.size() != decay.size()) throw std::runtime_error("begin_transient: beta and decay need one entry per precursor family each");
        if (beta.size() > NF_PRECURSORS_MAX) throw std::runtime_error("begin_transient: at most " + std::to_string(NF_PRECURSORS_MAX) + " precursor families");
        nf_kinetics kin{};
        kin.n_families = (int)beta.size();
        for (int i = 0; i < kin.n_families; ++i) { kin.beta[i] = beta.data()[i]; kin.lambda[i] = decay.data()[i]; }
        kin.velocity_host = velocity.data();
        arr_t cd;
        if (!chi_delayed.is_none()) {
            cd = chi_delayed.cast<arr_t>();
            if (cd.size() != ng_) throw std::runtime_error("begin_transient: chi_delayed needs one entry per group");
            kin.chi_delayed_host = cd.data();
        }
        chk(nf_set_phi(h_, Phi_.data()));
        chk(nf_transient_begin(h_, &kin, keff.is_none() ? last_keff_ : keff.cast<double>()));
        transient_ = nf_transient_result{}; transient_.power = 1.0; has_transient_ = true;
    }
    py::array_t<double> StepTransient(double dt, int n_steps)
    {
        need_built("step_transient");
        Log(VerbosityLevel::NORMAL, "\n=== CINETIQUE ESPACE-TEMPS (EULER IMPLICITE) ===");
        nf_keff_opts o = make_opts(false, {}, false);
        py::array_t<double> power((py::ssize_t)std::max(n_steps, 0));
        nf_transient_result r{};
        const int rc = nf_transient_step(h_, &o, dt, n_steps, n_steps > 0 ? power.mutable_data() : nullptr, &r);
        if (has_transient_ && (rc == NF_OK || rc == NF_ERR_NUMERIC)) { transient_ = r; if (r.n_steps > 0 && h_) (void)nf_get_phi(h_, Phi_.data()); }
        chk(rc);
        if (verb_ >= VerbosityLevel::NORMAL)
            std::cout << "  t = " << r.time << " : P/P0 = " << std::fixed << std::setprecision(8) << r.power << std::defaultfloat << "  (" << r.n_outer
                      << " iterations externes, max " << r.n_outer_max << " par pas" << (r.n_unconverged ? ", non converge" : "") << ")" << std::endl;
        return power;
    }
    py::array_t<double> GetPrecursors(int i)
    {
        need_built("get_precursors");
        std::vector<double> full((size_t)nphi_);
        chk(nf_get_precursors(h_, i, full.data()));
        std::vector<py::ssize_t> shape;
        if (dim_ >= 3) shape.push_back(nz_);
        if (dim_ >= 2) shape.push_back(ny_);
        shape.push_back(nx_);
        py::array_t<double> out(shape);                           // DOF 0 of every cell, shaped like one group of get_flux()
        double *po = out.mutable_data();
        for (long e = 0; e < ne_; ++e) po[e] = full[(size_t)e * nloc_];
        return out;
    }
    py::dict GetTransientInfo() const
    {
        if (!has_transient_) throw std::runtime_error("get_transient_info: call begin_transient() first");
        const nf_transient_result &r = transient_;
        py::dict d;
        d["time"] = r.time; d["power"] = r.power; d["production"] = r.production; d["phi_int"] = r.phi_int; d["precursors"] = r.precursors;
        d["rebalance"] = r.rebalance; d["n_steps"] = r.n_steps; d["n_outer"] = r.n_outer; d["n_outer_max"] = r.n_outer_max;
        d["cg_total"] = r.cg_total; d["n_unconverged"] = r.n_unconverged;
        return d;
    }
    // Adjoint-weighted kinetics parameters (extension; include/neutfem_hip.h, nf_kinetics_params / nf_transient_kinetics).
    // kinetics_parameters evaluates the solved flux with k = last_keff_ and the fields of the host mirrors, pushed the way sensitivity_maps
    // pushes them; get_transient_kinetics the running transient's own state with the adjoint flux of the mirror.  Both return the
    // nf_pk_result as a dict (the arrays cut to n_families) and change neither mirror.
    static py::dict PkDict(const nf_pk_result &r)
    {
        py::dict d;
        d["rho"] = r.rho; d["rho_dollars"] = r.rho_dollars; d["beta_eff"] = r.beta_eff; d["gen_time"] = r.gen_time; d["fw"] = r.fw;
        d["production"] = r.production; d["delayed_production"] = r.delayed_production; d["removal_leakage"] = r.removal_leakage;
        d["scatter"] = r.scatter; d["amplitude"] = r.amplitude; d["keff"] = r.keff; d["time"] = r.time;
        d["n_families"] = r.n_families; d["from_transient"] = r.from_transient;
        py::list bi, ca;
        for (int i = 0; i < r.n_families; ++i) { bi.append(r.beta_eff_i[i]); ca.append(r.c_amp[i]); }
        d["beta_eff_i"] = bi; d["c_amp"] = ca;
        return d;
    }
    py::dict KineticsParameters(arr_t velocity, arr_t beta, arr_t decay, py::object chi_delayed)
    {
        if (!h_) throw std::runtime_error("kinetics_parameters: call BuildMatrices() first (there is no CPU fallback)");
        if (!has_valid_keff_ || !has_valid_adjoint_)
            throw std::runtime_error(std::string("kinetics_parameters: call ") + (!has_valid_keff_ ? "SolveKeff()" : "SolveAdjoint()") +
                                     " first (the parameters need a solved flux, a solved adjoint flux and k-eff)");
        if (velocity.size() != ng_) throw std::runtime_error("kinetics_parameters: velocity needs one entry per group");
        if (beta.size() != decay.size()) throw std::runtime_error("kinetics_parameters: beta and decay need one entry per precursor family each");
        if (beta.size() > NF_PRECURSORS_MAX) throw std::runtime_error("kinetics_parameters: at most " + std::to_string(NF_PRECURSORS_MAX) + " precursor families");
        nf_kinetics kin{};
        kin.n_families = (int)beta.size();
        for (int i = 0; i < kin.n_families; ++i) { kin.beta[i] = beta.data()[i]; kin.lambda[i] = decay.data()[i]; }
        kin.velocity_host = velocity.data();
        arr_t cd;
        if (!chi_delayed.is_none()) {
            cd = chi_delayed.cast<arr_t>();
            if (cd.size() != ng_) throw std::runtime_error("kinetics_parameters: chi_delayed needs one entry per group");
            kin.chi_delayed_host = cd.data();
        }
        chk(nf_set_phi(h_, Phi_.data())); chk(nf_set_phi_adj(h_, PhiAdj_.data()));
        nf_pk_result r{};
        chk(nf_kinetics_params(h_, &kin, last_keff_, &r));
        return PkDict(r);
    }
    py::dict GetTransientKinetics()
    {
        if (!h_) throw std::runtime_error("get_transient_kinetics: call BuildMatrices() first (there is no CPU fallback)");
        if (!has_transient_) throw std::runtime_error("get_transient_kinetics: call begin_transient() first");
        if (!has_valid_adjoint_) throw std::runtime_error("get_transient_kinetics: call SolveAdjoint() first (the parameters are weighted with the adjoint flux)");
        chk(nf_set_phi_adj(h_, PhiAdj_.data()));
        nf_pk_result r{};
        chk(nf_transient_kinetics(h_, &r));
        return PkDict(r);
    }
    // SolveModes (extension; include/neutfem_hip.h, nf_solve_modes): the n_modes leading lambda-modes by block power iteration with the
    // tolerances and the linear solver of this object; returns the eigenvalues, descending.  Flux, adjoint flux and GetLastKeff stay as they are
    std::vector<double> SolveModes(int n_modes, int n_guard, bool adjoint)
    {
        need_built("SolveModes");
        Log(VerbosityLevel::NORMAL, adjoint ? "\n=== MODES LAMBDA (ADJOINT) ===" : "\n=== MODES LAMBDA (DIRECT) ===");
        nf_keff_opts o = make_opts(false, {}, false);
        nf_modes_result r{};
        chk(nf_solve_modes(h_, &o, n_modes, n_guard, adjoint ? 1 : 0, &r));
        modes_[adjoint ? 1 : 0] = r; has_modes_[adjoint ? 1 : 0] = true; last_modes_ = adjoint ? 1 : 0;
        if (verb_ >= VerbosityLevel::NORMAL) {
            std::cout << "  " << r.n_outer << " iterations externes, bloc de " << r.n_block << (r.converged ? "" : " (non converge)") << std::endl;
            for (int i = 0; i < r.n_modes; ++i)
                std::cout << "  k[" << i << "] = " << std::fixed << std::setprecision(8) << r.k[i] << std::defaultfloat << "  residu = " << r.residual[i] << std::endl;
        }
        return std::vector<double>(r.k, r.k + r.n_modes);
    }
    py::array_t<double> GetMode(int i, bool adjoint)
    {
        need_built("get_mode");
        std::vector<double> full((size_t)ng_ * nphi_);
        chk(nf_get_mode(h_, i, adjoint ? 1 : 0, full.data()));
        std::vector<py::ssize_t> shape; shape.push_back(ng_);
        if (dim_ >= 3) shape.push_back(nz_);
        if (dim_ >= 2) shape.push_back(ny_);
        shape.push_back(nx_);
        py::array_t<double> out(shape);                           // the cell means, shaped like get_flux()
        double *o = out.mutable_data();
        for (int g = 0; g < ng_; ++g) for (long e = 0; e < ne_; ++e) o[g * ne_ + e] = full[g * nphi_ + e * nloc_];
        return out;
    }
    py::dict GetModesInfo() const
    {
        if (last_modes_ < 0) throw std::runtime_error("get_modes_info: call SolveModes() first");
        const nf_modes_result &r = modes_[last_modes_];
        py::dict d;
        d["k"] = std::vector<double>(r.k, r.k + r.n_modes); d["residual"] = std::vector<double>(r.residual, r.residual + r.n_modes);
        d["dominance_ratio"] = r.dominance_ratio; d["n_modes"] = r.n_modes; d["n_block"] = r.n_block; d["n_outer"] = r.n_outer;
        d["cg_total"] = r.cg_total; d["converged"] = r.converged; d["adjoint"] = last_modes_ == 1;
        return d;
    }
    std::pair<double, py::array_t<double>> SolveCoarse(const std::vector<int> &refine)
    {
        need_built("SolveCoarse");
        chk(nf_set_phi(h_, Phi_.data()));
        nf_keff_opts o = make_opts(true, refine, false);
        py::array_t<double> out((py::ssize_t)(ng_ * nphi_));
        double k = 1.0;
        chk(nf_solve_coarse(h_, &o, &k, out.mutable_data()));
        return {k, out};
    }
    double SolveAdjoint(bool normalize_to_direct, bool use_direct_keff)
    {
        need_built("SolveAdjoint");
        Log(VerbosityLevel::NORMAL, "\n=== CALCUL DE K-EFFECTIF (ADJOINT) ===");
        chk(nf_set_phi(h_, Phi_.data()));                         // the bi-orthonormalisation uses the direct flux
        chk(nf_set_warm_state(h_, has_valid_keff_ ? 1 : 0, last_keff_));
        nf_keff_opts o = make_opts(false, {}, false);
        double k = 1.0; int nout = 0;
        chk(nf_solve_adjoint(h_, &o, normalize_to_direct ? 1 : 0, use_direct_keff ? 1 : 0, &k, &nout));
        chk(nf_get_phi_adj(h_, PhiAdj_.data()));
        if (verb_ >= VerbosityLevel::NORMAL) std::cout << "  k-eff adjoint = " << std::fixed << std::setprecision(8) << k << std::defaultfloat << std::endl;
        last_keff_adj_ = k; has_valid_adjoint_ = true;            // src/NeutFEM.cpp:2075
        return k;
    }
    void BuildDiagonalCache() { need_built("build_diagonal_cache"); chk(nf_build_diagonal_cache(h_)); }
    // ProjectFluxRefined / ProjectPowerRefined (include/NeutFEM.hpp:303-313, src/wrapper.cpp:1003-1043; declared, never defined there):
    // the exact mean of the flux polynomial over every sub-cell of the mesh refined by `refine` (read like SolveCoarse reads it,
    // src/NeutFEM.cpp:2396-2398).  The field is the host mirror (get_flux() / get_flux_adj()), pushed through the device flux, which
    // then gets Phi_ back as SolveKeff / SolveAdjoint / SolveCoarse push it.  One group at a time: the device holds N rx ry rz doubles.
    py::array_t<double> ProjectFlux(const std::vector<int> &refine, bool adjoint) { return project("project_flux", refine, adjoint, false); }
    py::array_t<double> ProjectPower(const std::vector<int> &refine, bool adjoint) { return project("project_power", refine, adjoint, true); }
    py::array_t<double> GetCurrent()
    {
        need_built("get_current");
        py::array_t<double> out((py::ssize_t)(ng_ * nJ_));
        chk(nf_get_J(h_, out.mutable_data()));
        return out;
    }
    std::map<int, int> GetBCMap() const { std::map<int, int> r; for (auto &kv : bc_types_) r[kv.first] = (int)kv.second; return r; }

    // ExportVTK (src/NeutFEM.cpp:2137-2332): legacy ASCII STRUCTURED_GRID, cell data.  Same dataset layout and field
    // names as the reference so existing ParaView states keep working; written on the host from the host mirrors
    // (flux, XS) and, for the cell-centred currents, from Sol_J_ fetched through nf_get_J.
    void ExportVTK(const std::string &filename, bool export_flux, bool export_current, bool export_xs, bool export_adjoint)
    {
        const std::string full = filename + ".vtk";
        std::ofstream f(full);
        if (!f.is_open()) throw std::runtime_error("Cannot open file: " + full);
        Log(VerbosityLevel::NORMAL, "Export VTK vers " + full);
        const long nc = ne_;
        f << "# vtk DataFile Version 3.0\n" << "NeutFEM Output - k-eff=" << std::fixed << std::setprecision(6) << last_keff_ << "\n"
          << "ASCII\nDATASET STRUCTURED_GRID\n" << "DIMENSIONS " << nx_ + 1 << " " << ny_ + 1 << " " << nz_ + 1 << "\n"
          << "POINTS " << (long)(nx_ + 1) * (ny_ + 1) * (nz_ + 1) << " double\n";
        for (int k = 0; k <= nz_; ++k) for (int j = 0; j <= ny_; ++j) for (int i = 0; i <= nx_; ++i)
            f << xb_[i] << " " << (dim_ >= 2 ? yb_[j] : 0.0) << " " << (dim_ == 3 ? zb_[k] : 0.0) << "\n";
        f << "\nCELL_DATA " << nc << "\n";
        auto scalars = [&](const std::string &name, const std::function<double(long)> &val) {
            f << "SCALARS " << name << " double 1\nLOOKUP_TABLE default\n";
            for (long e = 0; e < nc; ++e) f << val(e) << "\n";
        };
        if (export_flux) {
            for (int g = 0; g < ng_; ++g) scalars("Flux_g" + std::to_string(g), [&](long e) { return Phi_[g * nphi_ + e * nloc_]; });
            scalars("Flux_total", [&](long e) { double t = 0; for (int g = 0; g < ng_; ++g) t += Phi_[g * nphi_ + e * nloc_]; return t; });
        }
        if (export_adjoint && has_valid_adjoint_)                 // src/NeutFEM.cpp:2206-2214: only after a SolveAdjoint
            for (int g = 0; g < ng_; ++g) scalars("Flux_adj_g" + std::to_string(g), [&](long e) { return PhiAdj_[g * nphi_ + e * nloc_]; });
        if (export_current) {
            need_built("ExportVTK(export_current=True)");
            std::vector<double> J((size_t)ng_ * nJ_);
            chk(nf_get_J(h_, J.data()));
            int nf = 1; for (int t = 1; t < dim_; ++t) nf *= rt_ + 1;          // first DOF of every face (JxFaceIndex(..., local_dof = 0))
            const long njx = (long)(nx_ + 1) * ny_ * nz_ * nf, njy = dim_ >= 2 ? (long)nx_ * (ny_ + 1) * nz_ * nf : 0;
            for (int g = 0; g < ng_; ++g) {
                const double *Jg = J.data() + (size_t)g * nJ_;
                f << "VECTORS Current_g" << g << " double\n";
                for (int k = 0; k < nz_; ++k) for (int j = 0; j < ny_; ++j) for (int i = 0; i < nx_; ++i) {
                    const long fx = ((long)k * ny_ + j) * (nx_ + 1) + i;             // src/FEM.cpp:264-275
                    double jx = 0.5 * (Jg[fx * nf] + Jg[(fx + 1) * nf]), jy = 0.0, jz = 0.0;
                    if (dim_ >= 2) { const long fy = ((long)k * (ny_ + 1) + j) * nx_ + i; jy = 0.5 * (Jg[njx + fy * nf] + Jg[njx + (fy + nx_) * nf]); }
                    if (dim_ == 3) { const long fz = ((long)k * ny_ + j) * nx_ + i; jz = 0.5 * (Jg[njx + njy + fz * nf] + Jg[njx + njy + (fz + (long)nx_ * ny_) * nf]); }
                    f << jx << " " << jy << " " << jz << "\n";
                }
            }
        }
        if (export_xs) {
            const std::pair<const char *, const std::vector<double> *> fields[] = {
                {"D_g", &D_}, {"SigmaR_g", &SigR_}, {"NuSigF_g", &NSF_}, {"Chi_g", &Chi_}, {"KappaSigF_g", &KSF_}, {"Source_g", &SRC_}};
            for (auto &fd : fields)
                for (int g = 0; g < ng_; ++g) scalars(fd.first + std::to_string(g), [&](long e) { return (*fd.second)[g * nc + e]; });
            for (int gf = 0; gf < ng_; ++gf) for (int gt = 0; gt < ng_; ++gt)
                scalars("SigS_" + std::to_string(gf) + "_to_" + std::to_string(gt), [&](long e) { return SigS_[((size_t)gt * ng_ + gf) * nc + e]; });
        }
        f.close();
        Log(VerbosityLevel::NORMAL, "  Export termine: " + std::to_string(nc) + " cellules");
    }
    // ZoomResolved (include/NeutFEM.hpp:311, src/wrapper.cpp:1045-1065; declared, never defined there): the problem solved again on the
    // mesh refined by `refine` (clamped as project() clamps it) with the fission source of the coarse solution frozen.  k and the field
    // come from the host mirrors: last_keff_ / Phi_ after a SolveKeff, last_keff_adj_ / PhiAdj_ after a SolveAdjoint.  Returns the fine
    // cell means (DOF 0), (ng, [NZ,] [NY,] NX) like project_flux; changes neither mirror.
    py::array_t<double> ZoomResolved(const std::vector<int> &refine, bool adjoint)
    {
        // without a built device handle there is nothing to re-solve on, and there is no CPU fallback
        if (!h_) throw std::runtime_error("zoom_resolved: the re-solve is outside the accelerated hot path of neutfem_amd until the device "
                                          "handle is built (there is no CPU fallback): call BuildMatrices() first");
        if (adjoint ? !has_valid_adjoint_ : !has_valid_keff_)
            throw std::runtime_error(std::string("zoom_resolved: call ") + (adjoint ? "SolveAdjoint()" : "SolveKeff()") + " first (the zoom freezes the fission source of a solved "
                                     + (adjoint ? "adjoint " : "") + "flux and its k-eff)");
        const int rx = refine.size() > 0 ? std::max(refine[0], 1) : 1;
        const int ry = refine.size() > 1 && dim_ >= 2 ? std::max(refine[1], 1) : 1;
        const int rz = refine.size() > 2 && dim_ >= 3 ? std::max(refine[2], 1) : 1;
        Log(VerbosityLevel::NORMAL, "\n=== ZOOM RESOLU (SOURCES FIGEES) ===");
        chk(adjoint ? nf_set_phi_adj(h_, PhiAdj_.data()) : nf_set_phi(h_, Phi_.data()));
        nf_keff_opts o = make_opts(false, {}, false);
        struct Fine { nf_handle h = nullptr; ~Fine() { if (h) nf_destroy(h); } } fine;   // destroyed on every path out
        nf_zoom_result r{};
        chk(nf_zoom_resolved(h_, &o, rx, ry, rz, adjoint ? 1 : 0, adjoint ? last_keff_adj_ : last_keff_, &fine.h, &r));
        const long NX = (long)nx_ * rx, NY = (long)ny_ * ry, NZ = (long)nz_ * rz, NE = NX * NY * NZ;
        std::vector<double> phi((size_t)ng_ * NE * nloc_);
        chk(nf_get_phi(fine.h, phi.data()));
        std::vector<py::ssize_t> shape; shape.push_back(ng_);
        if (dim_ >= 3) shape.push_back(NZ);
        if (dim_ >= 2) shape.push_back(NY);
        shape.push_back(NX);
        py::array_t<double> out(shape);
        double *po = out.mutable_data();
        for (long i = 0; i < (long)ng_ * NE; ++i) po[i] = phi[(size_t)i * nloc_];    // host layout [g][E*nloc + p]: DOF 0 = the cell mean
        zoom_ = r; has_zoom_ = true;
        if (verb_ >= VerbosityLevel::NORMAL)
            std::cout << "  Zoom " << rx << " x " << ry << " x " << rz << " : " << r.n_outer << " iterations, " << r.cg_total << " iterations CG, "
                      << r.n_cells << " cellules" << (r.converged ? "" : " (non converge)") << std::endl;
        return out;
    }
    py::dict GetZoomInfo() const
    {
        if (!has_zoom_) throw std::runtime_error("get_zoom_info: call zoom_resolved() first");
        py::dict d;
        d["source"] = zoom_.source; d["phi_int"] = zoom_.phi_int; d["production"] = zoom_.production; d["n_outer"] = zoom_.n_outer;
        d["cg_total"] = zoom_.cg_total; d["converged"] = zoom_.converged; d["n_cells"] = zoom_.n_cells;
        return d;
    }

    // sensitivity_maps (extension): dk/dXS per cell by first-order perturbation theory (nf_sensitivity) with k = last_keff_
    // and the fields of the host mirrors Phi_ / PhiAdj_, pushed to the device the way zoom_resolved pushes them.  A dict of arrays shaped
    // like get_D() .. get_SigS(); changes neither mirror.
    py::dict SensitivityMaps()
    {
        if (!h_) throw std::runtime_error("sensitivity_maps: call BuildMatrices() first (there is no CPU fallback)");
        if (!has_valid_keff_ || !has_valid_adjoint_)
            throw std::runtime_error(std::string("sensitivity_maps: call ") + (!has_valid_keff_ ? "SolveKeff()" : "SolveAdjoint()") +
                                     " first (the maps need a solved flux, a solved adjoint flux and k-eff)");
        Log(VerbosityLevel::NORMAL, "\n=== CARTES DE SENSIBILITE (dk/dXS) ===");
        chk(nf_set_phi(h_, Phi_.data())); chk(nf_set_phi_adj(h_, PhiAdj_.data()));
        const size_t n1 = (size_t)ng_ * ne_, n2 = n1 * ng_;
        struct DevBuf { nf_handle h; void *p = nullptr; ~DevBuf() { if (p) nf_dev_free(h, p); } } buf{h_};
        chk(nf_dev_alloc(h_, (4 * n1 + n2) * sizeof(double), &buf.p));
        double *d = static_cast<double *>(buf.p);
        nf_sens_result r{};
        chk(nf_sensitivity(h_, last_keff_, d, d + n1, d + 2 * n1, d + 3 * n1, d + 4 * n1, &r));
        std::vector<py::ssize_t> shape; shape.push_back(ng_);
        if (dim_ >= 3) shape.push_back(nz_);
        if (dim_ >= 2) shape.push_back(ny_);
        shape.push_back(nx_);
        std::vector<py::ssize_t> shape2(shape); shape2.insert(shape2.begin(), ng_);
        py::dict out;
        const char *names[5] = { "D", "SigR", "NSF", "Chi", "SigS" };
        for (int i = 0; i < 5; ++i) {
            py::array_t<double> a(i == 4 ? shape2 : shape);
            chk(nf_memcpy_d2h(h_, a.mutable_data(), d + (size_t)i * n1, (i == 4 ? n2 : n1) * sizeof(double)));
            out[names[i]] = a;
        }
        sens_ = r; has_sens_ = true;
        return out;
    }
    py::dict GetSensitivityInfo() const
    {
        if (!has_sens_) throw std::runtime_error("get_sensitivity_info: call sensitivity_maps() first");
        py::dict d;
        d["norm"] = sens_.norm; d["keff"] = sens_.keff; d["n_cells"] = sens_.n_cells;
        return d;
    }

    // SolveGPT (extension): the generalized adjoint of R = <numerator, phi> / <denominator, phi> (nf_solve_gpt) with
    // k = last_keff_ and the fields of the host mirrors, pushed the way sensitivity_maps pushes them.  The weights are shaped like get_D().
    double SolveGPT(py::array_t<double, py::array::c_style | py::array::forcecast> numerator,
                    py::array_t<double, py::array::c_style | py::array::forcecast> denominator)
    {
        if (!h_) throw std::runtime_error("SolveGPT: call BuildMatrices() first (there is no CPU fallback)");
        if (!has_valid_keff_ || !has_valid_adjoint_)
            throw std::runtime_error(std::string("SolveGPT: call ") + (!has_valid_keff_ ? "SolveKeff()" : "SolveAdjoint()") +
                                     " first (the generalized adjoint needs a solved flux, a solved adjoint flux and k-eff)");
        if ((long)numerator.size() != (long)ng_ * ne_ || (long)denominator.size() != (long)ng_ * ne_)
            throw std::runtime_error("SolveGPT: the weights must be shaped like get_D()");
        Log(VerbosityLevel::NORMAL, "\n=== ADJOINT GENERALISE (GPT) ===");
        chk(nf_set_phi(h_, Phi_.data())); chk(nf_set_phi_adj(h_, PhiAdj_.data()));
        nf_keff_opts o = make_opts(false, {}, false);
        nf_gpt_result r{};
        has_gpt_ = false;
        chk(nf_solve_gpt(h_, &o, last_keff_, numerator.data(), denominator.data(), &r));
        Gamma_.resize((size_t)ng_ * nphi_);
        chk(nf_get_gamma(h_, Gamma_.data()));
        gpt_ = r; has_gpt_ = true;
        return r.R;
    }
    py::array_t<double> GetGamma()
    {
        if (!has_gpt_) throw std::runtime_error("get_gamma: call SolveGPT() first");
        return flux(Gamma_, gammaP0_);
    }
    // (1/R) dR/dp per cell from the solved flux, the generalized adjoint on the handle and last_keff_ (nf_gpt_sensitivity): a dict of
    // arrays shaped like get_D() .. get_SigS(), plus the direct maps "Wa" / "Wb" of the weights, shaped like get_D()
    py::dict GptSensitivityMaps()
    {
        if (!h_) throw std::runtime_error("gpt_sensitivity_maps: call BuildMatrices() first (there is no CPU fallback)");
        if (!has_gpt_) throw std::runtime_error("gpt_sensitivity_maps: call SolveGPT() first");
        chk(nf_set_phi(h_, Phi_.data()));
        const size_t n1 = (size_t)ng_ * ne_, n2 = n1 * ng_;
        struct DevBuf { nf_handle h; void *p = nullptr; ~DevBuf() { if (p) nf_dev_free(h, p); } } buf{h_};
        chk(nf_dev_alloc(h_, (6 * n1 + n2) * sizeof(double), &buf.p));
        double *d = static_cast<double *>(buf.p);
        nf_sens_result r{};
        chk(nf_gpt_sensitivity(h_, last_keff_, d, d + n1, d + 2 * n1, d + 3 * n1, d + 6 * n1, d + 4 * n1, d + 5 * n1, &r));
        std::vector<py::ssize_t> shape; shape.push_back(ng_);
        if (dim_ >= 3) shape.push_back(nz_);
        if (dim_ >= 2) shape.push_back(ny_);
        shape.push_back(nx_);
        std::vector<py::ssize_t> shape2(shape); shape2.insert(shape2.begin(), ng_);
        py::dict out;
        const char *names[7] = { "D", "SigR", "NSF", "Chi", "Wa", "Wb", "SigS" };
        for (int i = 0; i < 7; ++i) {
            py::array_t<double> a(i == 6 ? shape2 : shape);
            chk(nf_memcpy_d2h(h_, a.mutable_data(), d + (size_t)i * n1, (i == 6 ? n2 : n1) * sizeof(double)));
            out[names[i]] = a;
        }
        gpt_norm_ = r.norm;
        return out;
    }
    py::dict GetGptInfo() const
    {
        if (!has_gpt_) throw std::runtime_error("get_gpt_info: call SolveGPT() first");
        py::dict d;
        d["R"] = gpt_.R; d["wa_phi"] = gpt_.wa_phi; d["wb_phi"] = gpt_.wb_phi; d["dgamma"] = gpt_.dgamma; d["ratio"] = gpt_.ratio;
        d["deflation"] = gpt_.deflation; d["norm"] = gpt_.norm; d["n_outer"] = gpt_.n_outer; d["cg_total"] = gpt_.cg_total;
        d["converged"] = gpt_.converged; d["keff"] = last_keff_; d["gamma_F_phi"] = gpt_norm_;
        return d;
    }

    // ---- numpy views (src/NeutFEM.cpp:2626-2730) ---------------------------------------------------
    py::array_t<double> view(std::vector<double> &v, bool sigs = false)
    {
        std::vector<py::ssize_t> shape; shape.push_back(ng_); if (sigs) shape.push_back(ng_);
        if (dim_ >= 3) shape.push_back(nz_);
        if (dim_ >= 2) shape.push_back(ny_);
        shape.push_back(nx_);
        std::vector<py::ssize_t> strides(shape.size()); py::ssize_t s = sizeof(double);
        for (int i = (int)shape.size() - 1; i >= 0; --i) { strides[i] = s; s *= shape[i]; }
        return py::array_t<double>(shape, strides, v.data(), py::cast(this));
    }
    py::array_t<double> flux(std::vector<double> &src, std::vector<double> &p0)
    {
        if (nloc_ == 1) return view(src);
        p0.resize(ng_ * ne_);
        for (int g = 0; g < ng_; ++g) for (long e = 0; e < ne_; ++e) p0[g * ne_ + e] = src[g * nphi_ + e * nloc_];
        return view(p0);
    }

    int dim_, nx_, ny_, nz_, ng_, rt_, p_, nloc_;
    long ne_, nphi_, nJ_, nJface_;
    std::vector<double> xb_, yb_, zb_, D_, SRC_, SigR_, NSF_, KSF_, Chi_, SigS_, Phi_, PhiAdj_, fluxP0_, fluxAdjP0_, Gamma_, gammaP0_;
    double last_keff_ = 1.0, last_keff_adj_ = 1.0;

private:
    void Log(VerbosityLevel lvl, const std::string &s) const { if (verb_ >= lvl) std::cout << s << std::endl; }
    void chk(int rc) const { if (rc != NF_OK) throw std::runtime_error(std::string("neutfem_amd: ") + nf_last_error()); }
    void ensure_handle()
    {
        if (h_) return;
        int dev = 0; if (const char *e = std::getenv("NEUTFEM_DEVICE")) dev = std::atoi(e);
        else if (const char *lr = std::getenv("LOCAL_RANK")) dev = std::atoi(lr) % std::max(1, nf_device_count());
        chk(nf_create(rt_, p_, ng_, (int)xb_.size(), xb_.data(), (int)yb_.size(), yb_.data(), (int)zb_.size(), zb_.data(), dev, &h_));
    }
    void need_built(const char *who) const { if (!h_) throw std::runtime_error(std::string(who) + ": call BuildMatrices() first"); }
    py::array_t<double> project(const char *who, const std::vector<int> &refine, bool adjoint, bool power)
    {
        need_built(who);
        const int rx = refine.size() > 0 ? std::max(refine[0], 1) : 1;
        const int ry = refine.size() > 1 && dim_ >= 2 ? std::max(refine[1], 1) : 1;
        const int rz = refine.size() > 2 && dim_ >= 3 ? std::max(refine[2], 1) : 1;
        const long NX = (long)nx_ * rx, NY = (long)ny_ * ry, NZ = (long)nz_ * rz, NE = NX * NY * NZ;
        std::vector<py::ssize_t> shape; if (!power) shape.push_back(ng_);
        if (dim_ >= 3) shape.push_back(NZ);
        if (dim_ >= 2) shape.push_back(NY);
        shape.push_back(NX);
        py::array_t<double> out(shape);
        struct DevBuf { nf_handle h; void *p = nullptr; ~DevBuf() { if (p) nf_dev_free(h, p); } } buf{h_};
        chk(nf_dev_alloc(h_, (size_t)NE * sizeof(double), &buf.p));
        double *d = static_cast<double *>(buf.p), *o = out.mutable_data();
        chk(nf_set_phi(h_, adjoint ? PhiAdj_.data() : Phi_.data()));
        int rc = NF_OK;
        if (power) rc = nf_project_power(h_, rx, ry, rz, 0, KSF_.data(), d);
        for (int g = 0; !power && g < ng_ && rc == NF_OK; ++g) {
            rc = nf_project_flux(h_, rx, ry, rz, 0, g, d);
            if (rc == NF_OK) rc = nf_memcpy_d2h(h_, o + (size_t)g * NE, d, (size_t)NE * sizeof(double));
        }
        if (power && rc == NF_OK) rc = nf_memcpy_d2h(h_, o, d, (size_t)NE * sizeof(double));
        if (adjoint) {                                            // the device flux gets the direct mirror back, after an error too
            const std::string err = rc == NF_OK ? std::string() : nf_last_error();
            chk(nf_set_phi(h_, Phi_.data()));
            if (rc != NF_OK) throw std::runtime_error("neutfem_amd: " + err);
        }
        chk(rc);
        return out;
    }

    nf_handle h_ = nullptr;
    std::vector<unsigned char> void_; double void_gamma_ = 0.0; bool void_on_handle_ = false;   // set_void: the mask (empty = none), on the handle since the last BuildMatrices
    std::map<int, BCType> bc_types_; std::map<int, double> bc_values_; std::map<int, std::pair<double, double>> robin_;
    LinearSolverType solver_ = LinearSolverType::BICGSTAB; bool solver_pushed_ = false;   // src/NeutFEM.cpp:126 vs solvers.cpp:68
    double tol_keff_ = 1e-5, tol_flux_ = 1e-5, tol_L2_ = 1e-5; int max_outer_ = 200, max_inner_ = 1000;
    VerbosityLevel verb_ = VerbosityLevel::NORMAL; double cmfd_omega_ = 1.0;
    bool has_valid_keff_ = false, has_valid_adjoint_ = false;
    nf_subcrit_result subcrit_{}; bool has_subcrit_ = false;     // the last SolveSubcritical (get_subcritical_info)
    nf_modes_result modes_[2]{}; bool has_modes_[2] = {false, false}; int last_modes_ = -1;   // the last SolveModes, direct / adjoint (get_modes_info)
    nf_zoom_result zoom_{}; bool has_zoom_ = false;               // the last zoom_resolved (get_zoom_info)
    nf_sens_result sens_{}; bool has_sens_ = false;               // the last sensitivity_maps (get_sensitivity_info)
    nf_gpt_result gpt_{}; bool has_gpt_ = false; double gpt_norm_ = 0.0;   // the last SolveGPT (get_gpt_info); <Gamma+, F phi> of the last gpt_sensitivity_maps
    nf_transient_result transient_{}; bool has_transient_ = false;   // the last step_transient (get_transient_info)
};

// SolveKeffBatch (extension; include/neutfem_hip.h, nf_solve_keff_batch): SolveKeff() on every object of the list, each with
// its own tolerances and linear solver; small meshes of one shape run in one launch, one workgroup each.  Every object is left as its
// own SolveKeff() leaves it (get_flux(), GetLastKeff()).  An object whose solve failed raises after the others have been accepted.
static nf_batch_result g_last_batch{}; static bool g_has_batch = false;
static std::vector<double> SolveKeffBatch(const std::vector<NeutFEM *> &solvers, bool use_coarse_init, const std::vector<int> &coarse_factors,
                                          bool use_diagonal_solver, bool use_cmfd)
{
    const int n = (int)solvers.size();
    if (n < 1) throw std::invalid_argument("SolveKeffBatch: an empty list");
    for (NeutFEM *s : solvers) if (!s) throw std::invalid_argument("SolveKeffBatch: None in the list");
    for (int i = 0; i < n; ++i) for (int j = 0; j < i; ++j) if (solvers[i] == solvers[j]) throw std::invalid_argument("SolveKeffBatch: the same object twice");
    std::vector<nf_keff_opts> o; std::vector<nf_handle> h;
    for (NeutFEM *s : solvers) { o.push_back(s->keff_prepare(use_coarse_init, coarse_factors, use_diagonal_solver, use_cmfd, "SolveKeffBatch")); h.push_back(s->handle()); }
    std::vector<double> k(n, 1.0); std::vector<int> nout(n, 0), st(n, NF_OK);
    nf_batch_result r{};
    for (NeutFEM *s : solvers) s->progress_on(true);
    const int rc = nf_solve_keff_batch(h.data(), n, o.data(), n, k.data(), nout.data(), st.data(), &r);
    for (NeutFEM *s : solvers) s->progress_on(false);
    const std::string err = rc != NF_OK ? std::string("neutfem_amd: ") + nf_last_error() : std::string();   // before any further call of the C ABI
    bool any = false; for (int i = 0; i < n; ++i) any |= st[i] != NF_OK;
    if (rc != NF_OK && !any) throw std::runtime_error(err);       // refused as a whole: nothing ran
    g_last_batch = r; g_has_batch = true;
    for (int i = 0; i < n; ++i) if (st[i] == NF_OK) k[i] = solvers[i]->keff_accept(k[i], nout[i]);
    if (rc != NF_OK) throw std::runtime_error(err);
    return k;
}
static py::dict GetBatchInfo()
{
    if (!g_has_batch) throw std::runtime_error("get_batch_info: call SolveKeffBatch() first");
    py::dict d;
    d["n_batched"] = g_last_batch.n_batched; d["n_sequential"] = g_last_batch.n_sequential; d["n_launches"] = g_last_batch.n_launches; d["variant"] = g_last_batch.variant;
    return d;
}

PYBIND11_MODULE(_neutfem_eigen, m)
{
    m.doc() = "neutfem_amd: MI355X-native drop-in for jujuC31/NeutFEM's neutfem._neutfem_eigen (src/wrapper.cpp)";
    m.attr("__backend__") = "hip-gfx950";
    m.def("device_count", &nf_device_count, "number of visible HIP devices");
    m.def("SolveKeffBatch", &SolveKeffBatch, py::arg("solvers"), py::arg("use_coarse_init") = false, py::arg("coarse_factors") = std::vector<int>{},
          py::arg("use_diagonal_solver") = false, py::arg("use_cmfd") = false,
          "extension: SolveKeff() on every NeutFEM object of the list, small meshes of one shape in one launch; returns the list of k");
    m.def("get_batch_info", &GetBatchInfo, "extension: the last SolveKeffBatch's nf_batch_result as a dict (n_batched, n_sequential, n_launches, variant)");

    py::enum_<VerbosityLevel>(m, "VerbosityLevel")
        .value("SILENT", VerbosityLevel::SILENT).value("NORMAL", VerbosityLevel::NORMAL)
        .value("VERBOSE", VerbosityLevel::VERBOSE).value("DEBUG", VerbosityLevel::DEBUG);
    py::enum_<BCType>(m, "BCType")
        .value("DIRICHLET", BCType::DIRICHLET).value("NEUMANN", BCType::NEUMANN).value("ROBIN", BCType::ROBIN)
        .value("MIRROR", BCType::MIRROR).value("PERIODIC", BCType::PERIODIC);
    py::enum_<BoundaryID>(m, "BoundaryID")
        .value("LEFT_1D", BoundaryID::LEFT_1D).value("RIGHT_1D", BoundaryID::RIGHT_1D)
        .value("LEFT_2D", BoundaryID::LEFT_2D).value("RIGHT_2D", BoundaryID::RIGHT_2D)
        .value("TOP_2D", BoundaryID::TOP_2D).value("BOTTOM_2D", BoundaryID::BOTTOM_2D)
        .value("FRONT_3D", BoundaryID::FRONT_3D).value("BACK_3D", BoundaryID::BACK_3D)
        .value("LEFT_3D", BoundaryID::LEFT_3D).value("RIGHT_3D", BoundaryID::RIGHT_3D)
        .value("TOP_3D", BoundaryID::TOP_3D).value("BOTTOM_3D", BoundaryID::BOTTOM_3D);
    py::enum_<LinearSolverType>(m, "LinearSolverType")
        .value("DIRECT_LU", LinearSolverType::DIRECT_LU).value("DIRECT_LLT", LinearSolverType::DIRECT_LLT)
        .value("DIRECT_LDLT", LinearSolverType::DIRECT_LDLT).value("CG", LinearSolverType::CG)
        .value("CG_DIAG", LinearSolverType::CG_DIAG).value("CG_ICHOL", LinearSolverType::CG_ICHOL)
        .value("BICGSTAB", LinearSolverType::BICGSTAB).value("BICGSTAB_DIAG", LinearSolverType::BICGSTAB_DIAG)
        .value("BICGSTAB_ILU", LinearSolverType::BICGSTAB_ILU).value("LCG", LinearSolverType::LCG);

    py::class_<NeutFEM>(m, "NeutFEM")
        .def(py::init<int, int, arr_t, arr_t, arr_t>(), py::arg("order"), py::arg("ng"), py::arg("x_breaks"), py::arg("y_breaks"), py::arg("z_breaks"))
        .def(py::init<int, int, int, arr_t, arr_t, arr_t>(), py::arg("rt_order"), py::arg("p_order"), py::arg("ng"), py::arg("x_breaks"),
             py::arg("y_breaks"), py::arg("z_breaks"))
        .def("set_bc", &NeutFEM::SetBC, py::arg("attr"), py::arg("type"), py::arg("value") = 0.0)
        .def("set_robin_coefficients", &NeutFEM::SetRobin, py::arg("attr"), py::arg("alpha"), py::arg("beta"))
        .def("set_linear_solver", &NeutFEM::SetLinearSolver, py::arg("solver_type"))
        .def("set_tol", &NeutFEM::SetTolerance, py::arg("tol_keff"), py::arg("tol_flux"), py::arg("tol_L2"), py::arg("max_outer"), py::arg("max_inner"))
        .def("set_verbosity", &NeutFEM::SetVerbosity, py::arg("level"))
        .def("set_cmfd_relaxation", &NeutFEM::SetCMFDRelaxation, py::arg("omega"))
        .def("apply_quarter_symmetry", &NeutFEM::ApplyQuarterSymmetry, py::arg("axis1") = 0, py::arg("axis2") = 1)
        .def("add_refl", &NeutFEM::AddReflector, py::arg("D"), py::arg("SigR"), py::arg("SigS"))
        .def("set_refl", &NeutFEM::SetReflector, py::arg("refl_id"), py::arg("dimension"), py::arg("is_upper"))
        .def("clean_refl", &NeutFEM::ClearReflectors)
        .def("BuildMatrices", &NeutFEM::BuildMatrices)
        .def("SolveKeff", &NeutFEM::SolveKeff, py::arg("use_coarse_init") = false, py::arg("coarse_factors") = std::vector<int>{},
             py::arg("use_diagonal_solver") = false, py::arg("use_cmfd") = false)
        .def("SolveAdjoint", &NeutFEM::SolveAdjoint, py::arg("normalize_to_direct") = true, py::arg("use_direct_keff") = true)
        .def("SolveSubcritical", &NeutFEM::SolveSubcritical)
        .def("SolveModes", &NeutFEM::SolveModes, py::arg("n_modes"), py::arg("n_guard") = 2, py::arg("adjoint") = false,
             "extension: the n_modes leading lambda-modes by block power iteration; returns the list of k, descending")
        .def("get_mode", &NeutFEM::GetMode, py::arg("i"), py::arg("adjoint") = false,
             "extension: cell means of mode i of the last SolveModes of that kind, shaped like get_flux() (unit L2 norm over all DOFs)")
        .def("get_modes_info", &NeutFEM::GetModesInfo,
             "extension: the last SolveModes's nf_modes_result as a dict (k, residual, dominance_ratio, block size, outer counts, converged)")
        .def("SolveCoarse", &NeutFEM::SolveCoarse, py::arg("refine"))
        .def("build_diagonal_cache", &NeutFEM::BuildDiagonalCache)
        .def("initialize_cmfd", &NeutFEM::InitializeCMFD)
        .def("ExportVTK", &NeutFEM::ExportVTK, py::arg("filename"), py::arg("export_flux") = true, py::arg("export_current") = true,
             py::arg("export_xs") = false, py::arg("export_adjoint") = false)
        .def("ExportFluxVTK", [](NeutFEM &s, const std::string &fn, bool adj) { s.ExportVTK(fn, true, false, false, adj); }, py::arg("filename"), py::arg("adjoint") = false)
        .def("ExportXSVTK", [](NeutFEM &s, const std::string &fn) { s.ExportVTK(fn, false, false, true, false); }, py::arg("filename"))
        .def("get_D", [](NeutFEM &s) { return s.view(s.D_); })
        .def("get_SRC", [](NeutFEM &s) { return s.view(s.SRC_); })
        .def("get_SigR", [](NeutFEM &s) { return s.view(s.SigR_); })
        .def("get_NSF", [](NeutFEM &s) { return s.view(s.NSF_); })
        .def("get_KSF", [](NeutFEM &s) { return s.view(s.KSF_); })
        .def("get_Chi", [](NeutFEM &s) { return s.view(s.Chi_); })
        .def("get_SigS", [](NeutFEM &s) { return s.view(s.SigS_, true); })
        .def("get_flux", [](NeutFEM &s) { return s.flux(s.Phi_, s.fluxP0_); })
        .def("get_flux_adj", [](NeutFEM &s) { return s.flux(s.PhiAdj_, s.fluxAdjP0_); })
        .def("get_current", &NeutFEM::GetCurrent, "extension: Sol_J_ as a flat (ng*n_J) array in the reference DOF order")
        .def("set_void", &NeutFEM::SetVoid, py::arg("mask"), py::arg("gamma"),
             "extension: cut the cells with a non-zero mask entry (shaped like one group of get_D()) out of the domain, J.n = gamma phi on their faces to kept cells; takes effect at BuildMatrices()")
        .def("clear_void", &NeutFEM::ClearVoid, "extension: remove the set_void mask; takes effect at BuildMatrices()")
        .def("get_void", &NeutFEM::GetVoid, "extension: (mask as a bool array shaped like one group of get_D(), gamma) as set through set_void, None without a mask")
        .def("get_bc_map", &NeutFEM::GetBCMap, "extension: {attr: BCType value} as set through set_bc")
        .def("get_subcritical_info", &NeutFEM::GetSubcriticalInfo,
             "extension: the last SolveSubcritical's nf_subcrit_result as a dict (M, k_source, ratio, integrals, outer counts, converged)")
        .def("reset_flux", &NeutFEM::ResetFlux)
        .def("GetNumElements", [](const NeutFEM &s) { return s.ne_; })
        .def("GetNumGroups", [](const NeutFEM &s) { return s.nphi_ / s.ne_; })      // reference bug kept, src/wrapper.cpp:953-955
        .def("GetDimension", [](const NeutFEM &s) { return s.dim_; })
        .def("GetLastKeff", [](const NeutFEM &s) { return s.last_keff_; })
        .def("GetLastKeffAdjoint", [](const NeutFEM &s) { return s.last_keff_adj_; })
        .def("GetSolverName", &NeutFEM::GetSolverName)
        .def("project_flux", &NeutFEM::ProjectFlux, py::arg("refine"), py::arg("adjoint") = false,
             "mean flux of every sub-cell of the mesh refined by [rx, ry, rz]: (ng, [NZ,] [NY,] NX) like get_flux()")
        .def("project_power", &NeutFEM::ProjectPower, py::arg("refine"), py::arg("adjoint") = false,
             "sum over groups of get_KSF() times project_flux: ([NZ,] [NY,] NX), no normalisation")
        .def("zoom_resolved", &NeutFEM::ZoomResolved, py::arg("refine"), py::arg("adjoint") = false,
             "re-solve on the mesh refined by [rx, ry, rz] with the coarse fission source frozen: fine cell means (ng, [NZ,] [NY,] NX)")
        .def("get_zoom_info", &NeutFEM::GetZoomInfo,
             "extension: the last zoom_resolved's nf_zoom_result as a dict (source, phi_int, production, n_outer, cg_total, converged, n_cells)")
        .def("sensitivity_maps", &NeutFEM::SensitivityMaps,
             "extension: dk/dXS per cell from the solved flux, the solved adjoint flux and GetLastKeff(): {'D', 'SigR', 'NSF', 'Chi', 'SigS'} shaped like get_D() .. get_SigS()")
        .def("get_sensitivity_info", &NeutFEM::GetSensitivityInfo, "extension: the last sensitivity_maps' nf_sens_result as a dict (norm, keff, n_cells)")
        .def("SolveGPT", &NeutFEM::SolveGPT, py::arg("numerator"), py::arg("denominator"),
             "extension: the generalized adjoint of R = <numerator, phi> / <denominator, phi> (weights shaped like get_D()) at GetLastKeff(); returns R")
        .def("get_gamma", &NeutFEM::GetGamma, "extension: the generalized adjoint of the last SolveGPT, shaped like get_flux_adj()")
        .def("gpt_sensitivity_maps", &NeutFEM::GptSensitivityMaps,
             "extension: (1/R) dR/dp per cell: {'D', 'SigR', 'NSF', 'Chi', 'SigS'} shaped like get_D() .. get_SigS() and the direct maps 'Wa', 'Wb' of the weights")
        .def("get_gpt_info", &NeutFEM::GetGptInfo, "extension: the last SolveGPT's nf_gpt_result as a dict (R, sums, outers, converged, contraction, deflation residual)")
        .def("begin_transient", &NeutFEM::BeginTransient, py::arg("velocity"), py::arg("beta"), py::arg("decay"), py::arg("chi_delayed") = py::none(),
             py::arg("keff") = py::none(),
             "extension: start a transient from the current flux: velocity per group, beta / decay per precursor family, chi_delayed per group (None: Chi), keff (None: GetLastKeff())")
        .def("step_transient", &NeutFEM::StepTransient, py::arg("dt"), py::arg("n_steps") = 1,
             "extension: n_steps implicit-Euler steps of length dt; returns P / P(0) after every step; get_flux() then holds the flux at time t")
        .def("get_precursors", &NeutFEM::GetPrecursors, py::arg("i"), "extension: precursor family i of the running transient, cell values shaped like one group of get_flux()")
        .def("kinetics_parameters", &NeutFEM::KineticsParameters, py::arg("velocity"), py::arg("beta"), py::arg("decay"), py::arg("chi_delayed") = py::none(),
             "extension: adjoint-weighted rho, beta_eff (and its split), generation time and the raw forms of the solved flux at GetLastKeff() as a dict (arguments of begin_transient)")
        .def("get_transient_kinetics", &NeutFEM::GetTransientKinetics,
             "extension: the same for the running transient's own flux and precursors, with the data and keff of begin_transient")
        .def("get_transient_info", &NeutFEM::GetTransientInfo,
             "extension: the last step_transient's nf_transient_result as a dict (time, power, production, phi_int, precursors, rebalance, step and outer counts)");
}
