// ftmpc_multi.hip -- the batch axis across the GPUs of one node, inside ONE process.
//
// Instances are independent (the reference never couples them: one controller object per vehicle,
// ft_mpc/controllers/spiraling_mpc.py:288-317), so the batch is split contiguously: device g owns instances
// [B g / G, B (g+1) / G).  One host thread + one ftmpc_handle + one stream set per device; NO collective and
// nothing on xGMI: every worker reads its slice of the caller's arrays and writes its slice of the caller's
// outputs (that IS the "gather on the host").  Two ways to use it:
//   ftmpc_multi_solve_batch                   host buffers in / out, pinned staging per device (ftmpc_solve_batch)
//   ftmpc_multi_upload / _step / _download    shards stay RESIDENT in each device's HBM between steps
//                                             (what bench.py --gpus N times; Monte-Carlo campaigns)
// included by ftmpc_capi.hip (single translation unit).
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

#include <sched.h>

struct ftmpc_multi {
    struct Dev {
        int device = 0;
        ftmpc_handle* h = nullptr;
        std::thread th;
        int rc = 0;
        std::string err;
        // resident shard
        int64_t lo = 0, n = 0, cap = 0;
        bool has_warm = false, has_uref = false;
        int64_t xs = 0, us = 0, cap_xr = 0, cap_ur = 0;
        double *x0 = nullptr, *ub = nullptr, *stuck = nullptr, *xref = nullptr, *uref = nullptr, *warm = nullptr, *u0 = nullptr,
               *U = nullptr;
        int32_t *status = nullptr, *iters = nullptr;
        hipStream_t s = nullptr;
        // pinned staging of the resident upload: two halves, so that the host copy of one piece runs under the DMA of the other
        void* pin = nullptr;
        hipEvent_t pin_ev[2] = {nullptr, nullptr};
        int pin_turn = 0;
        int cpus_pinned = 0;     // host cores this device's worker thread is bound to (0: affinity left alone)
    };
    ftmpc_config cfg;
    std::vector<Dev> dev;
    std::mutex mu;
    std::condition_variable cv_job, cv_done;
    uint64_t gen = 0;
    int pending = 0;
    bool quit = false;
    std::function<int(ftmpc_multi::Dev&)> job;
    std::string err;
    int64_t B = 0;
};

namespace {

thread_local std::string g_multi_create_error;

// Binds the calling thread to the host cores nearest `device` (the PCI function's local_cpulist in sysfs, intersected with
// the cores this process may use); when the two do not meet -- containers often grant cores of one socket only -- the
// affinity is left alone.  Returns the number of cores bound to.
int pin_thread_near(int device) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) return 0;
    for (char* c = bus; *c; ++c)
        if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/local_cpulist";
    FILE* f = std::fopen(path.c_str(), "r");
    if (!f) return 0;
    char line[4096] = {0};
    const bool got = std::fgets(line, (int)sizeof(line), f) != nullptr;
    std::fclose(f);
    if (!got) return 0;
    cpu_set_t allowed, want;
    CPU_ZERO(&allowed);
    CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return 0;
    int n = 0;
    for (const char* p = line; *p;) {     // "0-15,128-143"
        char* end = nullptr;
        const long a = std::strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        p = end;
        if (*p == '-') {
            b = std::strtol(p + 1, &end, 10);
            p = end;
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c)
            if (c >= 0 && CPU_ISSET((int)c, &allowed)) {
                CPU_SET((int)c, &want);
                ++n;
            }
        while (*p == ',' || *p == ' ' || *p == '\n') ++p;
    }
    if (n == 0 || sched_setaffinity(0, sizeof(want), &want) != 0) return 0;
    return n;
}

void multi_worker(ftmpc_multi* m, int r) {
    ftmpc_multi::Dev& d = m->dev[r];
    (void)hipSetDevice(d.device);
    d.cpus_pinned = pin_thread_near(d.device);
    uint64_t seen = 0;
    for (;;) {
        std::function<int(ftmpc_multi::Dev&)> fn;
        {
            std::unique_lock<std::mutex> lk(m->mu);
            m->cv_job.wait(lk, [&] { return m->quit || m->gen != seen; });
            if (m->quit) return;
            seen = m->gen;
            fn = m->job;
        }
        const int rc = fn(d);
        {
            std::lock_guard<std::mutex> lk(m->mu);
            d.rc = rc;
            if (--m->pending == 0) m->cv_done.notify_all();
        }
    }
}

// runs fn on every device's thread at once and waits for all of them; first failing code wins
int multi_run(ftmpc_multi* m, std::function<int(ftmpc_multi::Dev&)> fn) {
    {
        std::lock_guard<std::mutex> lk(m->mu);
        m->job = std::move(fn);
        m->pending = (int)m->dev.size();
        ++m->gen;
    }
    m->cv_job.notify_all();
    std::unique_lock<std::mutex> lk(m->mu);
    m->cv_done.wait(lk, [&] { return m->pending == 0; });
    for (auto& d : m->dev)
        if (d.rc != FTMPC_OK) {
            m->err = "device " + std::to_string(d.device) + ": " + (d.err.empty() && d.h ? d.h->err : d.err);
            return d.rc;
        }
    return FTMPC_OK;
}

int dev_fail(ftmpc_multi::Dev& d, int code, const std::string& msg) {
    d.err = msg;
    return code;
}

template <typename T>
int dev_grow(ftmpc_multi::Dev& d, T** p, int64_t count) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    if (count <= 0) return FTMPC_OK;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), (size_t)count * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();   // clear the runtime's sticky "last error"
        return dev_fail(d, FTMPC_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    return FTMPC_OK;
}

#define DEV_TRY(d, expr)                                                                          \
    do {                                                                                          \
        hipError_t e__ = (expr);                                                                  \
        if (e__ != hipSuccess) return dev_fail((d), FTMPC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

// host -> device copy of a pageable array through the device's pinned staging halves (PIN_HALF bytes each)
constexpr size_t PIN_HALF = (size_t)8 << 20;
int dev_upload(ftmpc_multi::Dev& d, void* dst, const void* src, size_t bytes) {
    if (!d.pin) {      // all or nothing: a staging buffer without its two recorded events must not survive a failed set-up
        void* pin = nullptr;
        hipEvent_t ev[2] = {nullptr, nullptr};
        hipError_t e = hipHostMalloc(&pin, 2 * PIN_HALF, hipHostMallocDefault);
        for (int t = 0; t < 2 && e == hipSuccess; ++t) e = hipEventCreateWithFlags(&ev[t], hipEventDisableTiming);
        for (int t = 0; t < 2 && e == hipSuccess; ++t) e = hipEventRecord(ev[t], d.s);
        if (e != hipSuccess) {
            for (int t = 0; t < 2; ++t)
                if (ev[t]) (void)hipEventDestroy(ev[t]);
            if (pin) (void)hipHostFree(pin);
            (void)hipGetLastError();
            return dev_fail(d, FTMPC_ERR_HIP, std::string("pinned staging set-up: ") + hipGetErrorString(e));
        }
        d.pin = pin;
        d.pin_ev[0] = ev[0];
        d.pin_ev[1] = ev[1];
    }
    for (size_t off = 0; off < bytes; off += PIN_HALF) {
        const size_t cnt = std::min(PIN_HALF, bytes - off);
        const int t = d.pin_turn;
        d.pin_turn ^= 1;
        char* half = static_cast<char*>(d.pin) + (size_t)t * PIN_HALF;
        DEV_TRY(d, hipEventSynchronize(d.pin_ev[t]));       // the DMA that last read this half is done
        std::memcpy(half, static_cast<const char*>(src) + off, cnt);
        DEV_TRY(d, hipMemcpyAsync(static_cast<char*>(dst) + off, half, cnt, hipMemcpyHostToDevice, d.s));
        DEV_TRY(d, hipEventRecord(d.pin_ev[t], d.s));
    }
    return FTMPC_OK;
}

void shard(int64_t B, int G, int g, int64_t& lo, int64_t& hi) {
    lo = B * g / G;
    hi = B * (g + 1) / G;
}

// rows [T][n][w] of a shard's history into the caller's [T][B][w] at vehicle lo
template <typename V>
void scatter_rows(V* dst, const V* src, int64_t T, int64_t B, int64_t lo, int64_t n, int64_t w) {
    for (int64_t t = 0; t < T; ++t) std::memcpy(dst + (t * B + lo) * w, src + t * n * w, (size_t)(n * w) * sizeof(V));
}

// The closed loops over the device slots (ftmpc_multi_simulate_estimator_batch / _wrench_estimator_batch; hull_A == nullptr: the thruster
// form): slot g runs its shard [lo, hi) through the single-handle entry as the slice index0 = lo of a campaign of B, reading the
// caller's per-vehicle arrays at the shard's offset and writing the per-vehicle outputs there; a history goes through a shard-sized
// staging array and is copied row by row (one slot: straight into the caller's), the per-step counts are summed afterwards.
int multi_simulate(ftmpc_multi* m, const LoopCall& c) {
    if (!m) return FTMPC_ERR_ARG;
    const int64_t B = c.B;
    const int32_t T = c.T;
    auto refuse = [m](const std::string& msg) {
        m->err = msg;
        return FTMPC_ERR_ARG;
    };
    if (B < 0 || T < 0 || !c.x || !c.ub || !c.stuck || !c.noise || (c.wrench && (!c.hull_A || !c.hull_b || c.hull_rows < 1)))
        return refuse("null buffer or negative size");
    if (c.oc && c.oc->struct_size != (int32_t)sizeof(ftmpc_outcomes))
        return refuse("ftmpc_outcomes.struct_size is " + std::to_string(c.oc->struct_size) + ", this library expects " + std::to_string(sizeof(ftmpc_outcomes)));
    if (c.oc && (c.oc->index0 != 0 || (c.oc->index_total != 0 && c.oc->index_total != B)))
        return refuse("ftmpc_outcomes.index0 / index_total are set per device slot by the multi-GPU driver: pass 0 / 0 or 0 / B");
    if (c.fs && c.fs->struct_size != (int32_t)sizeof(ftmpc_fault_schedule)) return refuse("ftmpc_fault_schedule: bad struct_size");
    if (c.fs && (c.fs->n_events < 0 || c.fs->n_events > FTMPC_MAX_FAULT_EVENTS))
        return refuse("ftmpc_fault_schedule: n_events outside [0, FTMPC_MAX_FAULT_EVENTS]");
    {     // the plant model over the whole batch, so that a refusal names the vehicle by its number in the caller's arrays
        const std::string msg = plant_model_problem(c.pm, B, m->cfg.NT);
        if (!msg.empty()) return refuse(msg);
    }
    {     // the sensor likewise: the parameters are uniform, bias / pending and the two histories are per vehicle
        const std::string msg = sensor_problem(c.se, B, m->cfg.NT);
        if (!msg.empty()) return refuse(msg);
    }
    {     // the estimator likewise: the parameters are uniform, xhat / cov, est_hist and err_sq are per vehicle
        const std::string msg = estimator_problem(c.es, B);
        if (!msg.empty()) return refuse(msg);
    }
    if (c.dg) {     // the diagnosis likewise: the parameters are uniform, the state and the outputs per vehicle
        if (c.wrench) {
            const std::string msg = wrench_diagnosis_problem(c.fs, c.no_hull_step, B);
            if (!msg.empty()) return refuse(msg);
        }
        if (c.fs && c.fs->n_events > 0 && (!c.fs->onset || !c.fs->ub || !c.fs->stuck))
            return refuse("ftmpc_fault_schedule: null onset / ub / stuck");
        const std::string msg = diagnosis_problem(c.dg, B, m->cfg.NT, c.es, c.fs, c.se);
        if (!msg.empty()) return refuse(msg);
    }
    {     // the disturbance estimate likewise: the parameters are uniform, force / torque / cross / cov and the histories per vehicle
        const std::string msg = disturbance_problem(c.db, B, c.es, c.wrench ? 0 : c.sqp_iters);      // (the wrench SQP is served)
        if (!msg.empty()) return refuse(msg);
    }
    {     // the bias estimate likewise (thruster form only): the parameters are uniform, bias / cross / cov and the history per vehicle
        const std::string msg = bias_problem(c.be, B, c.es, c.db);
        if (!msg.empty()) return refuse(msg);
    }
    {     // the outage likewise: the parameters are uniform, window / state / rejected / outliers and the four histories per vehicle
        const std::string msg = outage_problem(c.og, B, c.es, c.db, c.be);
        if (!msg.empty()) return refuse(msg);
    }
    {     // the environment likewise: sigma, tau and period are uniform, every array is per vehicle
        const std::string msg = environment_problem(c.ev, B, c.se, c.db);
        if (!msg.empty()) return refuse(msg);
    }
    {     // the isolation likewise: consist, persist and revise are uniform, lead, the two counters and fit_hist per vehicle
        const std::string msg = isolation_problem(c.is, B, m->cfg.NT, c.dg);
        if (!msg.empty()) return refuse(msg);
    }
    {     // the mission likewise: tables are shared, table / offset / cost are per vehicle
        const std::string msg = mission_problem(c.ms, B, T, m->cfg.N, c.xref_traj, c.uref_traj, 0, sensor_shift(c.se));
        if (!msg.empty()) return refuse(msg);
    }
    {     // the actuator likewise: the parameters are uniform, delivered / pulses / state and the two histories are per vehicle.  (The
          // handle entry checks each shard's struct again, state included: what passed here cannot fail there.)
        const std::string msg = actuator_problem(c.ac, B, m->cfg.NT);
        if (!msg.empty()) return refuse(msg);
    }
    if (B == 0 || T == 0) {
        loop_empty(c, m->cfg.NT);
        return FTMPC_OK;
    }
    const int G = (int)m->dev.size();
    if (G > B) return refuse("more device slots (" + std::to_string(G) + ") than vehicles (B = " + std::to_string(B) + ")");
    const int NT = m->cfg.NT;
    std::vector<std::vector<int32_t>> bad((size_t)G), abad((size_t)G);      // per-slot counts per step
    const int rc = multi_run(m, [&](ftmpc_multi::Dev& d) -> int {
        const int g = (int)(&d - m->dev.data());
        int64_t lo, hi;
        shard(B, G, g, lo, hi);
        const int64_t n = hi - lo;
        ftmpc_fault_schedule fs{};
        if (c.fs) {
            fs = *c.fs;
            const int64_t E = fs.n_events;
            if (fs.onset) fs.onset += lo * E;
            if (fs.detect) fs.detect += lo * E;
            if (fs.ub) fs.ub += lo * E * NT;
            if (fs.stuck) fs.stuck += lo * E * NT;
            if (fs.hull_set) fs.hull_set += lo * E;
            if (fs.hull_b) fs.hull_b += lo * E * c.hull_rows;
        }
        ftmpc_plant_model pl{};
        if (c.pm) {
            pl = *c.pm;
            if (pl.mass) pl.mass += lo;
            if (pl.J) pl.J += lo * 9;
            if (pl.D) pl.D += lo * 6 * NT;
            if (pl.force) pl.force += lo * 3;
            if (pl.torque) pl.torque += lo * 3;
        }
        ftmpc_mission mi{};
        if (c.ms) {
            mi = *c.ms;
            if (mi.table) mi.table += lo;
            if (mi.offset) mi.offset += lo;
            if (mi.cost) mi.cost += lo * 3;
        }
        ftmpc_outcomes oc{};
        oc.struct_size = (int32_t)sizeof(ftmpc_outcomes);
        oc.index0 = lo;
        oc.index_total = B;
        const bool whole = n == B;      // one slot: no staging
        std::vector<double> uh, xh, ah;
        std::vector<int32_t> sh, kh;
        ftmpc_actuator at{};
        if (c.ac) {
            at = *c.ac;
            if (at.delivered) at.delivered += lo;
            if (at.pulses) at.pulses += lo;
            if (at.state) at.state += lo * NT;
        }
        std::vector<double> mh, ph;
        ftmpc_sensor sv{};
        if (c.se) {
            sv = *c.se;
            if (sv.bias) sv.bias += lo * 12;
            if (sv.pending) sv.pending += lo * sv.latency * NT;
        }
        std::vector<double> eh;
        ftmpc_estimator ev{};
        if (c.es) {
            ev = *c.es;
            if (ev.xhat) ev.xhat += lo * 13;
            if (ev.cov) ev.cov += lo * 78;
            if (ev.err_sq) ev.err_sq += lo * 4;
        }
        std::vector<double> lh;
        ftmpc_diagnosis dv{};
        if (c.dg) {
            dv = *c.dg;
            const int64_t K = dv.max_detect, H = (int64_t)NT * dv.n_levels;
            if (dv.state) dv.state += lo * (14 + NT);
            if (dv.llr) dv.llr += lo * H;
            if (dv.detect_step) dv.detect_step += lo * K;
            if (dv.detect_thruster) dv.detect_thruster += lo * K;
            if (dv.detect_level) dv.detect_level += lo * K;
            if (dv.ub) dv.ub += lo * NT;
            if (dv.stuck) dv.stuck += lo * NT;
        }
        std::vector<double> fh, th;
        ftmpc_disturbance bv{};
        if (c.db) {
            bv = *c.db;
            if (bv.force) bv.force += lo * 3;
            if (bv.torque) bv.torque += lo * 3;
            if (bv.cross) bv.cross += lo * 72;
            if (bv.cov) bv.cov += lo * 21;
        }
        std::vector<double> bh;
        ftmpc_bias_estimate sb{};
        if (c.be) {
            sb = *c.be;
            if (sb.bias) sb.bias += lo * 6;
            if (sb.cross) sb.cross += lo * 72;
            if (sb.cov) sb.cov += lo * 21;
        }
        std::vector<int32_t> oah, ooh, ogh;
        std::vector<double> omh;
        ftmpc_outage ov{};
        if (c.og) {
            ov = *c.og;
            if (ov.window) ov.window += lo * 2;
            if (ov.state) ov.state += lo * 3;
            if (ov.rejected) ov.rejected += lo * 4;
            if (ov.outliers) ov.outliers += lo * 4;
        }
        std::vector<double> ewh;
        ftmpc_environment nv{};
        if (c.ev) {
            nv = *c.ev;
            if (nv.amp_force) nv.amp_force += lo * 3;
            if (nv.amp_torque) nv.amp_torque += lo * 3;
            if (nv.phase) nv.phase += lo;
            if (nv.kick) nv.kick += lo * 6;
            if (nv.window) nv.window += lo * 2;
            if (nv.state) nv.state += lo * 6;
            if (nv.est_err_sq) nv.est_err_sq += lo * 2;
        }
        std::vector<double> ifh;
        ftmpc_isolation iv{};
        if (c.is) {
            iv = *c.is;
            if (iv.lead) iv.lead += lo * 2;
            if (iv.voided) iv.voided += lo;
            if (iv.revised) iv.revised += lo;
        }
        try {
            if (iv.fit_hist && !whole) ifh.resize((size_t)T * n * 2);
            if (nv.wrench_hist && !whole) ewh.resize((size_t)T * n * 6);
            if (ov.avail_hist && !whole) oah.resize((size_t)T * n);
            if (ov.outlier_hist && !whole) ooh.resize((size_t)T * n);
            if (ov.gate_hist && !whole) ogh.resize((size_t)T * n);
            if (ov.meas_hist && !whole) omh.resize((size_t)T * n * 13);
            if (sb.bias_hist && !whole) bh.resize((size_t)T * n * 6);
            if (bv.force_hist && !whole) fh.resize((size_t)T * n * 3);
            if (bv.torque_hist && !whole) th.resize((size_t)T * n * 3);
            if (dv.llr_hist && !whole) lh.resize((size_t)T * n * NT * dv.n_levels);
            if (ev.est_hist && !whole) eh.resize((size_t)T * n * 13);
            if (sv.meas_hist && !whole) mh.resize((size_t)T * n * 13);
            if (sv.pred_hist && !whole) ph.resize((size_t)T * n * 13);
            bad[g].assign((size_t)T, 0);
            abad[g].assign((size_t)T, 0);
            if (c.u_hist && !whole) uh.resize((size_t)T * n * NT);
            if (c.x_hist && !whole) xh.resize((size_t)T * n * 13);
            if (c.oc && c.oc->status_hist && !whole) sh.resize((size_t)T * n);
            if (at.applied_hist && !whole) ah.resize((size_t)T * n * NT);
            if (at.ticks_hist && !whole) kh.resize((size_t)T * n * NT);
        } catch (const std::bad_alloc&) {
            return dev_fail(d, FTMPC_ERR_ALLOC, "out of host memory for the shard's histories");
        }
        if (c.oc) {
            oc.tol_pos = c.oc->tol_pos;
            oc.tol_vel = c.oc->tol_vel;
            oc.tol_rate = c.oc->tol_rate;
            oc.err_int = c.oc->err_int ? c.oc->err_int + lo * 3 : nullptr;
            oc.err_max = c.oc->err_max ? c.oc->err_max + lo * 3 : nullptr;
            oc.impulse = c.oc->impulse ? c.oc->impulse + lo * 2 : nullptr;
            oc.settle_step = c.oc->settle_step ? c.oc->settle_step + lo : nullptr;
            oc.tset_step = c.oc->tset_step ? c.oc->tset_step + lo : nullptr;
            oc.unsolved = c.oc->unsolved ? c.oc->unsolved + lo : nullptr;
            oc.first_unsolved = c.oc->first_unsolved ? c.oc->first_unsolved + lo : nullptr;
            oc.alloc_failed = c.oc->alloc_failed ? c.oc->alloc_failed + lo : nullptr;
            oc.status_hist = !c.oc->status_hist ? nullptr : (whole ? c.oc->status_hist : sh.data());
        }
        double* const uh_p = !c.u_hist ? nullptr : (whole ? c.u_hist : uh.data());
        double* const xh_p = !c.x_hist ? nullptr : (whole ? c.x_hist : xh.data());
        if (!whole) {
            if (at.applied_hist) at.applied_hist = ah.data();
            if (at.ticks_hist) at.ticks_hist = kh.data();
            if (sv.meas_hist) sv.meas_hist = mh.data();
            if (sv.pred_hist) sv.pred_hist = ph.data();
            if (ev.est_hist) ev.est_hist = eh.data();
            if (dv.llr_hist) dv.llr_hist = lh.data();
            if (bv.force_hist) bv.force_hist = fh.data();
            if (bv.torque_hist) bv.torque_hist = th.data();
            if (sb.bias_hist) sb.bias_hist = bh.data();
            if (ov.avail_hist) ov.avail_hist = oah.data();
            if (ov.outlier_hist) ov.outlier_hist = ooh.data();
            if (ov.gate_hist) ov.gate_hist = ogh.data();
            if (ov.meas_hist) ov.meas_hist = omh.data();
            if (nv.wrench_hist) nv.wrench_hist = ewh.data();
            if (iv.fit_hist) iv.fit_hist = ifh.data();
        }
        LoopCall sc = c;      // the shard as a call of its own: the path of the single-handle entry
        sc.B = n;
        sc.x = c.x + lo * 13, sc.ub = c.ub + lo * NT, sc.stuck = c.stuck + lo * NT;
        if (c.wrench) {
            sc.hull_set = c.hull_set ? c.hull_set + lo : nullptr;
            sc.hull_b = c.hull_b + lo * c.hull_rows;
            sc.alloc_failed = c.alloc_failed ? abad[g].data() : nullptr;
            sc.out_hull_b = c.out_hull_b ? c.out_hull_b + lo * c.hull_rows : nullptr;
            sc.no_hull_step = c.no_hull_step ? c.no_hull_step + lo : nullptr;
        }
        sc.u_hist = uh_p, sc.x_hist = xh_p, sc.not_converged = bad[g].data();
        sc.fs = c.fs ? &fs : nullptr, sc.oc = &oc, sc.pm = c.pm ? &pl : nullptr, sc.ms = c.ms ? &mi : nullptr, sc.ac = c.ac ? &at : nullptr;
        sc.se = c.se ? &sv : nullptr, sc.es = c.es ? &ev : nullptr, sc.dg = c.dg ? &dv : nullptr, sc.db = c.db ? &bv : nullptr;
        sc.be = c.be ? &sb : nullptr;
        sc.og = c.og ? &ov : nullptr;
        sc.ev = c.ev ? &nv : nullptr;
        sc.is = c.is ? &iv : nullptr;
        const int rc2 = loop_run(d.h, sc);
        if (rc2 != FTMPC_OK) return dev_fail(d, rc2, ftmpc_last_error(d.h));
        if (!whole) {
            if (c.u_hist) scatter_rows(c.u_hist, uh.data(), T, B, lo, n, NT);
            if (c.x_hist) scatter_rows(c.x_hist, xh.data(), T, B, lo, n, 13);
            if (c.oc && c.oc->status_hist) scatter_rows(c.oc->status_hist, sh.data(), T, B, lo, n, 1);
            if (c.ac && c.ac->applied_hist) scatter_rows(c.ac->applied_hist, ah.data(), T, B, lo, n, NT);
            if (c.ac && c.ac->ticks_hist) scatter_rows(c.ac->ticks_hist, kh.data(), T, B, lo, n, NT);
            if (c.se && c.se->meas_hist) scatter_rows(c.se->meas_hist, mh.data(), T, B, lo, n, 13);
            if (c.se && c.se->pred_hist) scatter_rows(c.se->pred_hist, ph.data(), T, B, lo, n, 13);
            if (c.es && c.es->est_hist) scatter_rows(c.es->est_hist, eh.data(), T, B, lo, n, 13);
            if (c.dg && c.dg->llr_hist) scatter_rows(c.dg->llr_hist, lh.data(), T, B, lo, n, (int64_t)NT * dv.n_levels);
            if (c.db && c.db->force_hist) scatter_rows(c.db->force_hist, fh.data(), T, B, lo, n, 3);
            if (c.db && c.db->torque_hist) scatter_rows(c.db->torque_hist, th.data(), T, B, lo, n, 3);
            if (c.be && c.be->bias_hist) scatter_rows(c.be->bias_hist, bh.data(), T, B, lo, n, 6);
            if (c.og && c.og->avail_hist) scatter_rows(c.og->avail_hist, oah.data(), T, B, lo, n, 1);
            if (c.og && c.og->outlier_hist) scatter_rows(c.og->outlier_hist, ooh.data(), T, B, lo, n, 1);
            if (c.og && c.og->gate_hist) scatter_rows(c.og->gate_hist, ogh.data(), T, B, lo, n, 1);
            if (c.og && c.og->meas_hist) scatter_rows(c.og->meas_hist, omh.data(), T, B, lo, n, 13);
            if (c.ev && c.ev->wrench_hist) scatter_rows(c.ev->wrench_hist, ewh.data(), T, B, lo, n, 6);
            if (c.is && c.is->fit_hist) scatter_rows(c.is->fit_hist, ifh.data(), T, B, lo, n, 2);
        }
        return FTMPC_OK;
    });
    if (rc != FTMPC_OK) return rc;
    for (int32_t t = 0; t < T; ++t) {
        int32_t nb = 0, na = 0;
        for (int g = 0; g < G; ++g) {
            nb += bad[g][t];
            na += abad[g][t];
        }
        if (c.not_converged) c.not_converged[t] = nb;
        if (c.alloc_failed) c.alloc_failed[t] = na;
    }
    return FTMPC_OK;
}

}  // namespace

extern "C" {

int ftmpc_multi_create(const ftmpc_config* cfg, const int32_t* device_ids, int32_t n_devices, ftmpc_multi** out) {
    if (!cfg || !out) return FTMPC_ERR_ARG;
    *out = nullptr;
    // the ABI guard of ftmpc_create, BEFORE the struct is copied: a caller built against an older, shorter ftmpc_config must be
    // told, not read past its end (nothing beyond struct_size's own offset is touched until it has been checked)
    if (cfg->struct_size != (int32_t)sizeof(ftmpc_config)) {
        g_multi_create_error = "ftmpc_config.struct_size = " + std::to_string(cfg->struct_size) + " but this library was built with sizeof(ftmpc_config) = " +
                               std::to_string(sizeof(ftmpc_config)) + " (fill the struct with ftmpc_default_config of the SAME header)";
        return FTMPC_ERR_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_multi_create_error = "no HIP device visible (this library has no CPU fallback)";
        return FTMPC_ERR_NODEVICE;
    }
    if (n_devices <= 0) n_devices = ndev;
    if (n_devices > 64) {
        g_multi_create_error = "more than 64 device slots";
        return FTMPC_ERR_ARG;
    }
    ftmpc_multi* m = new (std::nothrow) ftmpc_multi();
    if (!m) return FTMPC_ERR_ALLOC;
    m->cfg = *cfg;
    m->dev.resize((size_t)n_devices);
    for (int i = 0; i < n_devices; ++i) {
        m->dev[i].device = device_ids ? device_ids[i] : i;     // the same ordinal may appear twice (two handles on one GPU)
        if (m->dev[i].device < 0 || m->dev[i].device >= ndev) {
            g_multi_create_error = "device id out of range";
            delete m;
            return FTMPC_ERR_ARG;
        }
    }
    for (int i = 0; i < n_devices; ++i) m->dev[i].th = std::thread(multi_worker, m, i);
    // every handle is created by the thread that will drive it
    const int rc = multi_run(m, [m](ftmpc_multi::Dev& d) -> int {
        ftmpc_config c = m->cfg;
        c.device_id = d.device;
        int rc2 = ftmpc_create(&c, &d.h);
        if (rc2 != FTMPC_OK) return dev_fail(d, rc2, ftmpc_last_error(nullptr));
        DEV_TRY(d, hipStreamCreateWithFlags(&d.s, hipStreamNonBlocking));
        return FTMPC_OK;
    });
    if (rc != FTMPC_OK) {
        g_multi_create_error = m->err;
        ftmpc_multi_destroy(m);
        return rc;
    }
    *out = m;
    return FTMPC_OK;
}

int ftmpc_multi_destroy(ftmpc_multi* m) {
    if (!m) return FTMPC_OK;
    (void)multi_run(m, [](ftmpc_multi::Dev& d) -> int {
        void* ptrs[] = {d.x0, d.ub, d.stuck, d.xref, d.uref, d.warm, d.u0, d.U, d.status, d.iters};
        for (void* p : ptrs)
            if (p) (void)hipFree(p);
        if (d.pin) (void)hipHostFree(d.pin);
        for (hipEvent_t e : d.pin_ev)
            if (e) (void)hipEventDestroy(e);
        if (d.s) (void)hipStreamDestroy(d.s);
        if (d.h) (void)ftmpc_destroy(d.h);
        d.h = nullptr;
        return FTMPC_OK;
    });
    {
        std::lock_guard<std::mutex> lk(m->mu);
        m->quit = true;
    }
    m->cv_job.notify_all();
    for (auto& d : m->dev)
        if (d.th.joinable()) d.th.join();
    delete m;
    return FTMPC_OK;
}

const char* ftmpc_multi_last_error(const ftmpc_multi* m) { return m ? m->err.c_str() : g_multi_create_error.c_str(); }

int32_t ftmpc_multi_device_count(const ftmpc_multi* m) { return m ? (int32_t)m->dev.size() : 0; }

int32_t ftmpc_multi_worker_cpus(const ftmpc_multi* m, int32_t slot) {
    return (m && slot >= 0 && slot < (int32_t)m->dev.size()) ? m->dev[slot].cpus_pinned : 0;
}

int ftmpc_multi_shard_bounds(const ftmpc_multi* m, int64_t B, int32_t slot, int64_t* lo, int64_t* hi) {
    if (!m || !lo || !hi || slot < 0 || slot >= (int32_t)m->dev.size() || B < 0) return FTMPC_ERR_ARG;
    shard(B, (int)m->dev.size(), slot, *lo, *hi);
    return FTMPC_OK;
}

int ftmpc_multi_solve_batch(ftmpc_multi* m, int64_t B, const double* x0, const double* ub, const double* stuck,
                            const double* xref, int64_t xref_stride, const double* uref, int64_t uref_stride, double* warmU,
                            double* out_u0, double* out_U, int32_t* status, int32_t* iters) {
    if (!m) return FTMPC_ERR_ARG;
    if (B < 0 || !x0 || !ub || !stuck || !xref || !out_u0) {
        m->err = "null buffer or negative batch";
        return FTMPC_ERR_ARG;
    }
    if (B == 0) return FTMPC_OK;
    const int G = (int)m->dev.size();
    const int N = m->cfg.N, NT = m->cfg.NT;
    const int64_t nw = (int64_t)N * NT;
    return multi_run(m, [=](ftmpc_multi::Dev& d) -> int {
        const int g = (int)(&d - m->dev.data());
        int64_t lo, hi;
        shard(B, G, g, lo, hi);
        if (hi <= lo) return FTMPC_OK;
        return ftmpc_solve_batch(d.h, hi - lo, x0 + lo * 13, ub + lo * NT, stuck + lo * NT, xref + lo * xref_stride, xref_stride,
                                 uref ? uref + lo * uref_stride : nullptr, uref_stride, warmU ? warmU + lo * nw : nullptr,
                                 out_u0 + lo * NT, out_U ? out_U + lo * nw : nullptr, status ? status + lo : nullptr,
                                 iters ? iters + lo : nullptr);
    });
}

int ftmpc_multi_upload(ftmpc_multi* m, int64_t B, const double* x0, const double* ub, const double* stuck, const double* xref,
                       int64_t xref_stride, const double* uref, int64_t uref_stride, const double* warmU) {
    if (!m) return FTMPC_ERR_ARG;
    if (B <= 0 || !x0 || !ub || !stuck || !xref) {
        m->err = "null buffer or empty batch";
        return FTMPC_ERR_ARG;
    }
    const int N = m->cfg.N, NT = m->cfg.NT;
    if ((xref_stride != 0 && xref_stride < 9 * (N + 1)) || (uref && uref_stride != 0 && uref_stride < 6 * (N + 1))) {
        m->err = "reference strides must be 0 or at least one window";
        return FTMPC_ERR_ARG;
    }
    const int G = (int)m->dev.size();
    const int64_t nw = (int64_t)N * NT;
    m->B = B;
    return multi_run(m, [=](ftmpc_multi::Dev& d) -> int {
        const int g = (int)(&d - m->dev.data());
        int64_t lo, hi;
        shard(B, G, g, lo, hi);
        const int64_t n = hi - lo;
        d.lo = lo;
        d.n = n;
        d.has_warm = warmU != nullptr;
        d.has_uref = uref != nullptr;
        d.xs = xref_stride;
        d.us = uref_stride;
        if (n <= 0) return FTMPC_OK;
        int rc;
        if (n > d.cap) {
            d.cap = 0;   // nothing is usable until every buffer below exists again (a failure part-way must not leave a stale capacity)
            if ((rc = dev_grow(d, &d.x0, n * 13)) || (rc = dev_grow(d, &d.ub, n * NT)) || (rc = dev_grow(d, &d.stuck, n * NT)) ||
                (rc = dev_grow(d, &d.warm, n * nw)) || (rc = dev_grow(d, &d.u0, n * NT)) || (rc = dev_grow(d, &d.U, n * nw)) ||
                (rc = dev_grow(d, &d.status, n)) || (rc = dev_grow(d, &d.iters, n)))
                return rc;
            d.cap = n;
        }
        const int64_t nxr = xref_stride == 0 ? 9 * (N + 1) : n * xref_stride;
        const int64_t nur = !uref ? 0 : (uref_stride == 0 ? 6 * (N + 1) : n * uref_stride);
        if (nxr > d.cap_xr) {
            d.cap_xr = 0;
            if ((rc = dev_grow(d, &d.xref, nxr))) return rc;
            d.cap_xr = nxr;
        }
        if (nur > d.cap_ur) {
            d.cap_ur = 0;
            if ((rc = dev_grow(d, &d.uref, nur))) return rc;
            d.cap_ur = nur;
        }
        if ((rc = ftmpc_reserve(d.h, n)) != FTMPC_OK) return dev_fail(d, rc, ftmpc_last_error(d.h));
        // the caller's arrays are pageable: through the pinned halves, so that the DMA engine streams instead of the
        // runtime's own bounce copies
        if ((rc = dev_upload(d, d.x0, x0 + lo * 13, (size_t)n * 13 * 8)) || (rc = dev_upload(d, d.ub, ub + lo * NT, (size_t)n * NT * 8)) ||
            (rc = dev_upload(d, d.stuck, stuck + lo * NT, (size_t)n * NT * 8)) ||
            (rc = dev_upload(d, d.xref, xref + lo * xref_stride, (size_t)nxr * 8)))
            return rc;
        if (uref && (rc = dev_upload(d, d.uref, uref + lo * uref_stride, (size_t)nur * 8))) return rc;
        if (warmU && (rc = dev_upload(d, d.warm, warmU + lo * nw, (size_t)n * nw * 8))) return rc;
        DEV_TRY(d, hipStreamSynchronize(d.s));
        return FTMPC_OK;
    });
}

int ftmpc_multi_step(ftmpc_multi* m, int32_t steps, int32_t keep_U) {
    if (!m || steps < 0) return FTMPC_ERR_ARG;
    if (m->B <= 0) {
        m->err = "nothing uploaded";
        return FTMPC_ERR_ARG;
    }
    return multi_run(m, [=](ftmpc_multi::Dev& d) -> int {
        if (d.n <= 0) return FTMPC_OK;
        for (int s = 0; s < steps; ++s) {
            const int rc = ftmpc_solve_batch_device(d.h, d.n, d.x0, d.ub, d.stuck, d.xref, d.xs, d.has_uref ? d.uref : nullptr, d.us,
                                                    d.has_warm ? d.warm : nullptr, d.u0, keep_U ? d.U : nullptr, d.status, d.iters, d.s);
            if (rc != FTMPC_OK) return dev_fail(d, rc, ftmpc_last_error(d.h));
        }
        DEV_TRY(d, hipStreamSynchronize(d.s));
        return FTMPC_OK;
    });
}

int ftmpc_multi_download(ftmpc_multi* m, double* out_u0, double* out_U, int32_t* status, int32_t* iters) {
    if (!m) return FTMPC_ERR_ARG;
    if (m->B <= 0) {
        m->err = "nothing uploaded";
        return FTMPC_ERR_ARG;
    }
    const int N = m->cfg.N, NT = m->cfg.NT;
    const int64_t nw = (int64_t)N * NT;
    return multi_run(m, [=](ftmpc_multi::Dev& d) -> int {
        if (d.n <= 0) return FTMPC_OK;
        if (out_u0) DEV_TRY(d, hipMemcpyAsync(out_u0 + d.lo * NT, d.u0, (size_t)d.n * NT * 8, hipMemcpyDeviceToHost, d.s));
        if (out_U) DEV_TRY(d, hipMemcpyAsync(out_U + d.lo * nw, d.U, (size_t)d.n * nw * 8, hipMemcpyDeviceToHost, d.s));
        if (status) DEV_TRY(d, hipMemcpyAsync(status + d.lo, d.status, (size_t)d.n * 4, hipMemcpyDeviceToHost, d.s));
        if (iters) DEV_TRY(d, hipMemcpyAsync(iters + d.lo, d.iters, (size_t)d.n * 4, hipMemcpyDeviceToHost, d.s));
        DEV_TRY(d, hipStreamSynchronize(d.s));
        return FTMPC_OK;
    });
}

int ftmpc_multi_simulate_outcomes_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                        const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                        int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                        double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out) {
    return ftmpc_multi_simulate_plant_batch(m, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults,
                                            u_hist, x_hist, not_converged, out, nullptr);
}

int ftmpc_multi_simulate_plant_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                     const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                     int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                     double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                     const ftmpc_plant_model* plant) {
    return ftmpc_multi_simulate_mission_batch(m, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults,
                                              u_hist, x_hist, not_converged, out, plant, nullptr);
}

int ftmpc_multi_simulate_mission_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                       const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                       int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                       double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                       const ftmpc_plant_model* plant, const ftmpc_mission* mission) {
    return ftmpc_multi_simulate_actuator_batch(m, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults,
                                               u_hist, x_hist, not_converged, out, plant, mission, nullptr);
}

int ftmpc_multi_simulate_wrench_outcomes_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                               const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                               int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                               uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                               const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                               int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out) {
    return ftmpc_multi_simulate_wrench_plant_batch(m, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj,
                                                   noise, seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged,
                                                   alloc_failed, out, nullptr);
}

int ftmpc_multi_simulate_wrench_plant_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                            const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                            int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                            uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                            const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                            int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                            const ftmpc_plant_model* plant) {
    return ftmpc_multi_simulate_wrench_mission_batch(m, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj,
                                                     uref_traj, noise, seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist,
                                                     not_converged, alloc_failed, out, plant, nullptr);
}

int ftmpc_multi_simulate_wrench_mission_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                              const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                              int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                              uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                              const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                              int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                              const ftmpc_plant_model* plant, const ftmpc_mission* mission) {
    return ftmpc_multi_simulate_wrench_actuator_batch(m, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj,
                                                      uref_traj, noise, seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist,
                                                      not_converged, alloc_failed, out, plant, mission, nullptr);
}

int ftmpc_multi_simulate_actuator_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                        const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                        int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                        double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                        const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator) {
    return ftmpc_multi_simulate_sensor_batch(m, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults,
                                             u_hist, x_hist, not_converged, out, plant, mission, actuator, nullptr);
}

int ftmpc_multi_simulate_wrench_actuator_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                               const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                               int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                               uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                               const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                               int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                               const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                               const ftmpc_actuator* actuator) {
    return ftmpc_multi_simulate_wrench_sensor_batch(m, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj,
                                                    uref_traj, noise, seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist,
                                                    not_converged, alloc_failed, out, plant, mission, actuator, nullptr);
}

int ftmpc_multi_simulate_sensor_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                      const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                      int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                      double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                      const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                      const ftmpc_sensor* sensor) {
    return ftmpc_multi_simulate_estimator_batch(m, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol,
                                                faults, u_hist, x_hist, not_converged, out, plant, mission, actuator, sensor, nullptr);
}

int ftmpc_multi_simulate_wrench_sensor_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                             const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                             int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                             uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                             const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                             int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                             const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                             const ftmpc_actuator* actuator, const ftmpc_sensor* sensor) {
    return ftmpc_multi_simulate_wrench_estimator_batch(m, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj,
                                                       uref_traj, noise, seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist,
                                                       not_converged, alloc_failed, out, plant, mission, actuator, sensor, nullptr);
}

int ftmpc_multi_simulate_estimator_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                         const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                         int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                         double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                         const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                         const ftmpc_sensor* sensor, const ftmpc_estimator* estimator) {
    return ftmpc_multi_simulate_diagnosis_batch(m, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol,
                                                faults, u_hist, x_hist, not_converged, out, plant, mission, actuator, sensor, estimator,
                                                nullptr);
}

int ftmpc_multi_simulate_diagnosis_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                         const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                         int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                         double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                         const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                         const ftmpc_sensor* sensor, const ftmpc_estimator* estimator,
                                         const ftmpc_diagnosis* diagnosis) {
    return ftmpc_multi_simulate_disturbance_batch(m, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol,
                                                  faults, u_hist, x_hist, not_converged, out, plant, mission, actuator, sensor, estimator,
                                                  diagnosis, nullptr);
}

int ftmpc_multi_simulate_disturbance_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                           const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                           int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                           double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                           const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                           const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                           const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                           const ftmpc_disturbance* disturbance) {
    return ftmpc_multi_simulate_bias_batch(m, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults,
                                           u_hist, x_hist, not_converged, out, plant, mission, actuator, sensor, estimator, diagnosis,
                                           disturbance, nullptr);
}

int ftmpc_multi_simulate_bias_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                    const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                    int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                    double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                    const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                    const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                    const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                    const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate) {
    return ftmpc_multi_simulate_outage_batch(m, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults,
                                             u_hist, x_hist, not_converged, out, plant, mission, actuator, sensor, estimator, diagnosis,
                                             disturbance, bias_estimate, nullptr);
}

int ftmpc_multi_simulate_outage_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                      const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                      int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                      double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                      const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                      const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                      const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                      const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                                      const ftmpc_outage* outage) {
    return ftmpc_multi_simulate_environment_batch(m, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol,
                                                  faults, u_hist, x_hist, not_converged, out, plant, mission, actuator, sensor, estimator,
                                                  diagnosis, disturbance, bias_estimate, outage, nullptr);
}

int ftmpc_multi_simulate_environment_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                           const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                           int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                           double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                           const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                           const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                           const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                           const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                                           const ftmpc_outage* outage, const ftmpc_environment* environment) {
    return ftmpc_multi_simulate_isolation_batch(m, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol,
                                                faults, u_hist, x_hist, not_converged, out, plant, mission, actuator, sensor, estimator,
                                                diagnosis, disturbance, bias_estimate, outage, environment, nullptr);
}

int ftmpc_multi_simulate_isolation_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                         const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                         int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                         double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                         const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                         const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                         const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                         const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                                         const ftmpc_outage* outage, const ftmpc_environment* environment,
                                         const ftmpc_isolation* isolation) {
    LoopCall c = loop_call(B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, u_hist, not_converged);
    loop_call_features(c, x_hist, faults, out, plant, mission, actuator, sensor, estimator, diagnosis, disturbance, bias_estimate, outage,
                       environment, isolation);
    return multi_simulate(m, c);
}

int ftmpc_multi_simulate_wrench_estimator_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                                const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                                int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                                uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                                const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                                int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                                const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                                const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                                const ftmpc_estimator* estimator) {
    return ftmpc_multi_simulate_wrench_diagnosis_batch(m, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj,
                                                       uref_traj, noise, seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist,
                                                       not_converged, alloc_failed, out, plant, mission, actuator, sensor, estimator,
                                                       nullptr, nullptr, nullptr);
}

int ftmpc_multi_simulate_wrench_diagnosis_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                                const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                                int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                                uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                                const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                                int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                                const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                                const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                                const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                                int32_t* no_hull_step) {
    return ftmpc_multi_simulate_wrench_disturbance_batch(m, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj,
                                                         uref_traj, noise, seed, sqp_iters, backtracks, tol, penalty, faults, u_hist,
                                                         x_hist, not_converged, alloc_failed, out, plant, mission, actuator, sensor,
                                                         estimator, diagnosis, out_hull_b, no_hull_step, nullptr);
}

int ftmpc_multi_simulate_wrench_disturbance_batch(ftmpc_multi* m, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                                  const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                                  int32_t hull_rows, const double* xref_traj, const double* uref_traj,
                                                  const double noise[4], uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol,
                                                  double penalty, const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                                  int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                                  const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                                  const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                                  const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                                  int32_t* no_hull_step, const ftmpc_disturbance* disturbance) {
    LoopCall c = loop_call(B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, u_hist, not_converged);
    loop_call_wrench(c, hull_A, n_sets, hull_set, hull_b, hull_rows, penalty, alloc_failed);
    c.out_hull_b = out_hull_b;
    c.no_hull_step = no_hull_step;
    loop_call_features(c, x_hist, faults, out, plant, mission, actuator, sensor, estimator, diagnosis, disturbance, nullptr);
    return multi_simulate(m, c);
}

const char* ftmpc_multi_routed_kernel_name(const ftmpc_multi* m, int32_t slot) {
    return (m && !m->dev.empty()) ? ftmpc_routed_kernel_name(m->dev[0].h, slot) : ftmpc_kernel_name(slot);
}

int ftmpc_multi_set_profiling(ftmpc_multi* m, int32_t enabled) {
    if (!m) return FTMPC_ERR_ARG;
    for (auto& d : m->dev) (void)ftmpc_set_profiling(d.h, enabled);
    return FTMPC_OK;
}

int ftmpc_multi_last_kernel_ms(ftmpc_multi* m, int32_t slot, float* ms, int32_t n_slots) {
    if (!m || !ms || slot < 0 || slot >= (int32_t)m->dev.size()) return FTMPC_ERR_ARG;
    return multi_run(m, [=](ftmpc_multi::Dev& d) -> int {
        if ((int)(&d - m->dev.data()) != slot) return FTMPC_OK;
        const int rc = ftmpc_last_kernel_ms(d.h, ms, n_slots);
        return rc == FTMPC_OK ? rc : dev_fail(d, rc, ftmpc_last_error(d.h));
    });
}

}  // extern "C"
