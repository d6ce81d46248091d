// The host layer of the on-device closed loops (included by ftmpc_capi.hip; ftmpc_multi.hip builds on it): the argument checks of the
// feature structs, one description of a call (LoopCall), a stage struct per feature that owns the feature's buffers, the loop itself
// (simulate_core) and the public ftmpc_simulate_* entries.  No kernel lives here.
#include "ftmpc_pack.h"

namespace {

// Every argument of a closed-loop call.  The public entries fill one, the multi-GPU driver one per shard.
struct LoopCall {
    int64_t B = 0;
    int32_t T = 0;
    double* x = nullptr;                  // [B][13], in/out
    const double* ub = nullptr;
    const double* stuck = nullptr;
    const double* xref_traj = nullptr;
    const double* uref_traj = nullptr;
    const double* noise = nullptr;        // [4]
    uint64_t seed = 0;
    int32_t sqp_iters = 0, backtracks = 0;
    double tol = 0.0;
    double penalty = 0.0;                 // the wrench SQP's merit weight (sqp_iters > 0)
    // the two-stage structure inside the closed loop: hull tables staged once (wrench_prepare), constant over the run
    bool wrench = false;
    const double* hull_A = nullptr;
    int32_t n_sets = 0;
    const int32_t* hull_set = nullptr;    // per vehicle, or null: one table
    const double* hull_b = nullptr;
    int32_t hull_rows = 0;
    int32_t* alloc_failed = nullptr;      // host [T] or null
    double* out_hull_b = nullptr;         // host [B*hull_rows] or null: the controller's offsets after the last step
    int32_t* no_hull_step = nullptr;      // host [B] or null, in/out (under a diagnosis): the step of the first detection that left no hull
    double* u_hist = nullptr;
    double* x_hist = nullptr;
    int32_t* not_converged = nullptr;
    const ftmpc_fault_schedule* fs = nullptr;
    const ftmpc_outcomes* oc = nullptr;
    const ftmpc_plant_model* pm = nullptr;
    const ftmpc_mission* ms = nullptr;
    const ftmpc_actuator* ac = nullptr;
    const ftmpc_sensor* se = nullptr;
    const ftmpc_estimator* es = nullptr;
    const ftmpc_diagnosis* dg = nullptr;
    const ftmpc_disturbance* db = nullptr;
    const ftmpc_bias_estimate* be = nullptr;
    const ftmpc_outage* og = nullptr;
    const ftmpc_environment* ev = nullptr;
    const ftmpc_isolation* is = nullptr;
    const ftmpc_probe* pb = nullptr;
};

// the thruster lead-in and the wrench lead-in of the public entries, which differ in nothing else
LoopCall loop_call(int64_t B, int32_t T, double* x, const double* ub, const double* stuck, const double* xref_traj, const double* uref_traj,
                   const double* noise, uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double* u_hist,
                   int32_t* not_converged) {
    LoopCall c;
    c.B = B, c.T = T, c.x = x, c.ub = ub, c.stuck = stuck, c.xref_traj = xref_traj, c.uref_traj = uref_traj, c.noise = noise, c.seed = seed;
    c.sqp_iters = sqp_iters, c.backtracks = backtracks, c.tol = tol, c.u_hist = u_hist, c.not_converged = not_converged;
    return c;
}
void loop_call_wrench(LoopCall& c, const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                      double penalty, int32_t* alloc_failed) {
    c.wrench = true;
    c.hull_A = hull_A, c.n_sets = n_sets, c.hull_set = hull_set, c.hull_b = hull_b, c.hull_rows = hull_rows;
    c.penalty = penalty, c.alloc_failed = alloc_failed;
}

// A plant model's layout and values (include/ftmpc.h, ftmpc_plant_model) over the vehicles [0, B): empty when it is acceptable, else the
// message, which names the field and the first offending vehicle (first: number of vehicle 0 in the caller's batch)
std::string plant_model_problem(const ftmpc_plant_model* pm, int64_t B, int NT, int64_t first = 0) {
    if (!pm) return "";
    if (pm->struct_size != (int32_t)sizeof(ftmpc_plant_model))
        return "ftmpc_plant_model.struct_size is " + std::to_string(pm->struct_size) + ", this library expects " +
               std::to_string(sizeof(ftmpc_plant_model));
    auto at = [first](const char* field, int64_t b, const std::string& what) {
        return std::string("ftmpc_plant_model.") + field + ": vehicle " + std::to_string(first + b) + " " + what;
    };
    if (pm->mass)
        for (int64_t b = 0; b < B; ++b)
            if (!std::isfinite(pm->mass[b]) || !(pm->mass[b] > 0.0)) return at("mass", b, "is not finite and positive");
    if (pm->J)
        for (int64_t b = 0; b < B; ++b) {
            const double* J = pm->J + b * 9;
            double big = 0.0;
            for (int k = 0; k < 9; ++k) {
                if (!std::isfinite(J[k])) return at("J", b, "has a non-finite entry");
                big = std::max(big, std::fabs(J[k]));
            }
            for (int i = 0; i < 3; ++i)
                for (int j = i + 1; j < 3; ++j)
                    if (std::fabs(J[3 * i + j] - J[3 * j + i]) > 1e-12 * big) return at("J", b, "is not symmetric");
            const double m2 = J[0] * J[4] - J[1] * J[3];
            const double m3 = J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]) + J[2] * (J[3] * J[7] - J[4] * J[6]);
            if (!(J[0] > 0.0) || !(m2 > 0.0) || !(m3 > 0.0)) return at("J", b, "is not positive definite");
        }
    const double* const arr[3] = {pm->D, pm->force, pm->torque};
    const char* const name[3] = {"D", "force", "torque"};
    const int64_t per[3] = {6 * (int64_t)NT, 3, 3};
    for (int a = 0; a < 3; ++a)
        if (arr[a])
            for (int64_t i = 0; i < B * per[a]; ++i)
                if (!std::isfinite(arr[a][i])) return at(name[a], i / per[a], "has a non-finite entry");
    return "";
}
int check_plant(ftmpc_handle* h, int64_t B, const ftmpc_plant_model* pm) {
    const std::string msg = plant_model_problem(pm, B, h->cfg.NT);
    return msg.empty() ? FTMPC_OK : fail(h, FTMPC_ERR_ARG, msg);
}

// A mission's layout and values (include/ftmpc.h, ftmpc_mission) over the vehicles [0, B) of a loop of T steps with horizon N, together
// with the call's own xref_traj / uref_traj: empty when acceptable, else the message, which names the field and, where there is one,
// the first offending vehicle (first: number of vehicle 0 in the caller's batch)
std::string mission_problem(const ftmpc_mission* ms, int64_t B, int32_t T, int N, const double* xref_traj, const double* uref_traj,
                                   int64_t first = 0, int L = 0) {
    if (!ms) return xref_traj ? "" : "null buffer or negative size";
    if (ms->struct_size != (int32_t)sizeof(ftmpc_mission))
        return "ftmpc_mission.struct_size is " + std::to_string(ms->struct_size) + ", this library expects " +
               std::to_string(sizeof(ftmpc_mission));
    if (ms->n_tables < 0) return "ftmpc_mission.n_tables is negative";
    if (ms->n_tables == 0) {
        if (!xref_traj) return "ftmpc_mission.n_tables = 0: every vehicle tracks the call's xref_traj, which is NULL";
        if (ms->table) return "ftmpc_mission.table is given, but n_tables = 0 (no table to choose from)";
        if (ms->offset) return "ftmpc_mission.offset is given, but n_tables = 0 (the call's xref_traj has no start column)";
        return "";
    }
    // (L: the columns a predicting sensor shifts every window by, ftmpc_sensor)
    const int64_t K = ms->n_tables, C = ms->n_cols, need = (int64_t)T + N + L;
    const std::string sum = L > 0 ? "T + N + L = " : "T + N = ";
    if (!ms->xref) return "ftmpc_mission.xref is NULL with n_tables = " + std::to_string(K);
    if (C < need)
        return "ftmpc_mission.n_cols = " + std::to_string(C) + " is below " + sum + std::to_string(need);
    if (xref_traj) return "ftmpc_mission.n_tables > 0: the call's xref_traj must be NULL (the tables are the reference)";
    if (uref_traj) return "ftmpc_mission.n_tables > 0: the call's uref_traj must be NULL (ftmpc_mission.uref holds the tables' uref)";
    auto at = [first](const char* field, int64_t b, const std::string& what) {
        return std::string("ftmpc_mission.") + field + ": vehicle " + std::to_string(first + b) + " " + what;
    };
    if (ms->table)
        for (int64_t b = 0; b < B; ++b)
            if (ms->table[b] < 0 || ms->table[b] >= K)
                return at("table", b, "has table " + std::to_string(ms->table[b]) + ", outside [0, " + std::to_string(K) + ")");
    if (ms->offset)
        for (int64_t b = 0; b < B; ++b) {
            if (ms->offset[b] < 0) return at("offset", b, "has a negative start column");
            if ((int64_t)ms->offset[b] + need > C)
                return at("offset", b, "has offset + " + sum + std::to_string((int64_t)ms->offset[b] + need) + " beyond n_cols = " +
                                           std::to_string(C));
        }
    const double* const arr[2] = {ms->xref, ms->uref};
    const char* const name[2] = {"xref", "uref"};
    const int64_t rows[2] = {9, 6};
    for (int a = 0; a < 2; ++a)
        if (arr[a])
            for (int64_t i = 0; i < K * rows[a] * C; ++i)
                if (!std::isfinite(arr[a][i]))
                    return std::string("ftmpc_mission.") + name[a] + ": table " + std::to_string(i / (rows[a] * C)) +
                           " has a non-finite entry in column " + std::to_string(i % (rows[a] * C) / rows[a]);
    return "";
}
int check_mission(ftmpc_handle* h, int64_t B, int32_t T, const ftmpc_mission* ms, const double* xref_traj, const double* uref_traj,
                         int L = 0) {
    const std::string msg = mission_problem(ms, B, T, h->cfg.N, xref_traj, uref_traj, 0, L);
    return msg.empty() ? FTMPC_OK : fail(h, FTMPC_ERR_ARG, msg);
}
// cost of a loop without steps: zero
void zero_mission_cost(const ftmpc_mission* ms, int64_t B) {
    if (ms && ms->cost && B > 0) std::fill(ms->cost, ms->cost + 3 * B, 0.0);
}

// An actuator's layout and values (include/ftmpc.h, ftmpc_actuator) over the vehicles [0, B): empty when acceptable, else the message,
// which names the field and, where there is one, the first offending vehicle (first: number of vehicle 0 in the caller's batch)
std::string actuator_problem(const ftmpc_actuator* ac, int64_t B, int NT, int64_t first = 0) {
    if (!ac) return "";
    if (ac->struct_size != (int32_t)sizeof(ftmpc_actuator))
        return "ftmpc_actuator.struct_size is " + std::to_string(ac->struct_size) + ", this library expects " +
               std::to_string(sizeof(ftmpc_actuator));
    if (ac->mode != 0 && ac->mode != 1) return "ftmpc_actuator.mode is " + std::to_string(ac->mode) + ", outside {0, 1}";
    if (ac->substeps < 0 || ac->substeps > 64) return "ftmpc_actuator.substeps is " + std::to_string(ac->substeps) + ", outside [0, 64]";
    const int S = ac->substeps > 0 ? ac->substeps : 1;
    if (ac->min_on < 0 || ac->min_on > S)
        return "ftmpc_actuator.min_on is " + std::to_string(ac->min_on) + ", outside [0, S = " + std::to_string(S) + "]";
    if (ac->align < 0 || ac->align > 2) return "ftmpc_actuator.align is " + std::to_string(ac->align) + ", outside {0, 1, 2}";
    if (!std::isfinite(ac->tau_on) || ac->tau_on < 0) return "ftmpc_actuator.tau_on is negative or not finite";
    if (!std::isfinite(ac->tau_off) || ac->tau_off < 0) return "ftmpc_actuator.tau_off is negative or not finite";
    if (ac->mode == 0) {
        if (ac->min_on != 0) return "ftmpc_actuator.min_on is given, but mode = 0 (a proportional valve has no dead band)";
        if (ac->align != 0) return "ftmpc_actuator.align is given, but mode = 0 (a proportional valve has no pulse to align)";
        if (ac->pulses) return "ftmpc_actuator.pulses is given, but mode = 0 (a proportional valve has no pulses)";
        if (ac->ticks_hist) return "ftmpc_actuator.ticks_hist is given, but mode = 0 (a proportional valve has no ticks)";
    }
    if (ac->state)
        for (int64_t i = 0; i < B * NT; ++i)
            if (!std::isfinite(ac->state[i]) || ac->state[i] < 0)
                return "ftmpc_actuator.state: vehicle " + std::to_string(first + i / NT) + " has a negative or non-finite valve state (thruster " +
                       std::to_string(i % NT) + ")";
    return "";
}
int check_actuator(ftmpc_handle* h, int64_t B, const ftmpc_actuator* ac) {
    const std::string msg = actuator_problem(ac, B, h->cfg.NT);
    return msg.empty() ? FTMPC_OK : fail(h, FTMPC_ERR_ARG, msg);
}
// trivial: the loop launches the plant kernels it launches without the struct
bool actuator_trivial(const ftmpc_actuator* ac) {
    return !ac || (ac->mode == 0 && ac->substeps <= 1 && ac->tau_on == 0 && ac->tau_off == 0 && !ac->delivered && !ac->pulses &&
                   !ac->applied_hist && !ac->ticks_hist && !ac->state);
}
// the sums of a loop without steps: zero (the valve states stay as they are)
void zero_actuator_sums(const ftmpc_actuator* ac, int64_t B) {
    if (ac && ac->delivered && B > 0) std::fill(ac->delivered, ac->delivered + B, 0.0);
    if (ac && ac->pulses && B > 0) std::fill(ac->pulses, ac->pulses + B, 0);
}

// A sensor's layout and values (include/ftmpc.h, ftmpc_sensor) over the vehicles [0, B): empty when acceptable, else the message, which
// names the field and, for an array, the first offending vehicle (first: number of vehicle 0 in the caller's batch)
std::string sensor_problem(const ftmpc_sensor* se, int64_t B, int NT, int64_t first = 0) {
    if (!se) return "";
    if (se->struct_size != (int32_t)sizeof(ftmpc_sensor))
        return "ftmpc_sensor.struct_size is " + std::to_string(se->struct_size) + ", this library expects " + std::to_string(sizeof(ftmpc_sensor));
    if (se->latency < 0 || se->latency > FTMPC_MAX_LATENCY)
        return "ftmpc_sensor.latency is " + std::to_string(se->latency) + ", outside [0, " + std::to_string(FTMPC_MAX_LATENCY) + "]";
    if (se->predict != 0 && se->predict != 1) return "ftmpc_sensor.predict is " + std::to_string(se->predict) + ", outside {0, 1}";
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(se->sigma[k]) || se->sigma[k] < 0)
            return "ftmpc_sensor.sigma[" + std::to_string(k) + "] is negative or not finite";
    if (se->step0 < 0) return "ftmpc_sensor.step0 is negative";
    if (se->pending && se->latency == 0) return "ftmpc_sensor.pending is given, but latency = 0 (no command waits)";
    if (se->pred_hist && se->predict == 0) return "ftmpc_sensor.pred_hist is given, but predict = 0 (nothing is predicted)";
    if (se->bias)
        for (int64_t i = 0; i < B * 12; ++i)
            if (!std::isfinite(se->bias[i]))
                return "ftmpc_sensor.bias: vehicle " + std::to_string(first + i / 12) + " has a non-finite entry (channel " +
                       std::to_string(i % 12) + ")";
    if (se->pending) {
        const int64_t per = (int64_t)se->latency * NT;
        for (int64_t i = 0; i < B * per; ++i)
            if (!std::isfinite(se->pending[i]))
                return "ftmpc_sensor.pending: vehicle " + std::to_string(first + i / per) + " has a non-finite entry (row " +
                       std::to_string(i % per / NT) + ")";
    }
    return "";
}
int check_sensor(ftmpc_handle* h, int64_t B, const ftmpc_sensor* se) {
    const std::string msg = sensor_problem(se, B, h->cfg.NT);
    return msg.empty() ? FTMPC_OK : fail(h, FTMPC_ERR_ARG, msg);
}
// trivial: the loop launches the kernels it launches without the struct
bool sensor_trivial(const ftmpc_sensor* se) {
    return !se || (se->latency == 0 && se->predict == 0 && se->sigma[0] == 0 && se->sigma[1] == 0 && se->sigma[2] == 0 && se->sigma[3] == 0 &&
                   !se->bias && !se->pending && !se->meas_hist && !se->pred_hist);
}
// columns a predicting sensor shifts every reference window by (0 for a struct that would be refused)
int sensor_shift(const ftmpc_sensor* se) {
    return se && se->predict == 1 && se->latency > 0 && se->latency <= FTMPC_MAX_LATENCY ? se->latency : 0;
}

// An estimator's layout and values (include/ftmpc.h, ftmpc_estimator) over the vehicles [0, B): empty when acceptable, else the
// message, which names the field and, for an array, the first offending vehicle (first: number of vehicle 0 in the caller's batch)
std::string estimator_problem(const ftmpc_estimator* es, int64_t B, int64_t first = 0) {
    if (!es) return "";
    if (es->struct_size != (int32_t)sizeof(ftmpc_estimator))
        return "ftmpc_estimator.struct_size is " + std::to_string(es->struct_size) + ", this library expects " +
               std::to_string(sizeof(ftmpc_estimator));
    if (es->every < 1) return "ftmpc_estimator.every is " + std::to_string(es->every) + ", below 1";
    for (int k = 0; k < 4; ++k) {
        if (!std::isfinite(es->p0[k]) || es->p0[k] < 0) return "ftmpc_estimator.p0[" + std::to_string(k) + "] is negative or not finite";
        if (!std::isfinite(es->proc_sigma[k]) || es->proc_sigma[k] < 0)
            return "ftmpc_estimator.proc_sigma[" + std::to_string(k) + "] is negative or not finite";
        if (!std::isfinite(es->meas_sigma[k]) || !(es->meas_sigma[k] > 0))
            return "ftmpc_estimator.meas_sigma[" + std::to_string(k) + "] is not finite and > 0";
    }
    if (es->cov && !es->xhat) return "ftmpc_estimator.cov is given without xhat";
    if (es->xhat)
        for (int64_t i = 0; i < B * 13; ++i)
            if (!std::isfinite(es->xhat[i]))
                return "ftmpc_estimator.xhat: vehicle " + std::to_string(first + i / 13) + " has a non-finite entry (" + std::to_string(i % 13) + ")";
    if (es->cov)
        for (int64_t b = 0; b < B; ++b) {
            const double* c = es->cov + b * 78;
            for (int k = 0; k < 78; ++k)
                if (!std::isfinite(c[k]))
                    return "ftmpc_estimator.cov: vehicle " + std::to_string(first + b) + " has a non-finite entry (" + std::to_string(k) + ")";
            for (int i = 0, k = 0; i < 12; k += 12 - i, ++i)
                if (c[k] < 0)
                    return "ftmpc_estimator.cov: vehicle " + std::to_string(first + b) + " has a negative diagonal entry (" + std::to_string(i) + ")";
        }
    return "";
}
// A disturbance estimate's layout and values (include/ftmpc.h, ftmpc_disturbance) over the vehicles [0, B), against the estimator and
// the SQP count: empty when acceptable, else the message
std::string disturbance_problem(const ftmpc_disturbance* db, int64_t B, const ftmpc_estimator* es, int32_t sqp_iters, int64_t first = 0) {
    if (!db) return "";
    if (db->struct_size != (int32_t)sizeof(ftmpc_disturbance))
        return "ftmpc_disturbance.struct_size is " + std::to_string(db->struct_size) + ", this library expects " +
               std::to_string(sizeof(ftmpc_disturbance));
    if (!es) return "ftmpc_disturbance needs an estimator (ftmpc_estimator): the disturbance states augment its filter";
    if (sqp_iters > 0) return "ftmpc_disturbance: sqp_iters must be 0 (the cost kernels of the SQP do not know the estimate)";
    if (db->compensate != 0 && db->compensate != 1) return "ftmpc_disturbance.compensate is " + std::to_string(db->compensate) + ", outside {0, 1}";
    for (int k = 0; k < 2; ++k) {
        if (!std::isfinite(db->p0[k]) || db->p0[k] < 0) return "ftmpc_disturbance.p0[" + std::to_string(k) + "] is negative or not finite";
        if (!std::isfinite(db->proc_sigma[k]) || db->proc_sigma[k] < 0)
            return "ftmpc_disturbance.proc_sigma[" + std::to_string(k) + "] is negative or not finite";
    }
    if (db->cross && !db->force) return "ftmpc_disturbance.cross is given without force";
    if (db->cross && !db->torque) return "ftmpc_disturbance.cross is given without torque";
    if (db->cross && !es->xhat) return "ftmpc_disturbance.cross is given without ftmpc_estimator.xhat";
    if (db->cov && !db->cross) return "ftmpc_disturbance.cov is given without cross";
    const double* const arr[4] = {db->force, db->torque, db->cross, db->cov};
    const char* const name[4] = {"force", "torque", "cross", "cov"};
    const int64_t width[4] = {3, 3, 72, 21};
    for (int a = 0; a < 4; ++a)
        if (arr[a])
            for (int64_t i = 0; i < B * width[a]; ++i)
                if (!std::isfinite(arr[a][i]))
                    return std::string("ftmpc_disturbance.") + name[a] + ": vehicle " + std::to_string(first + i / width[a]) +
                           " has a non-finite entry (" + std::to_string(i % width[a]) + ")";
    if (db->cov)
        for (int64_t b = 0; b < B; ++b)
            for (int i = 0, k = 0; i < 6; k += 6 - i, ++i)
                if (db->cov[b * 21 + k] < 0)
                    return "ftmpc_disturbance.cov: vehicle " + std::to_string(first + b) + " has a negative diagonal entry (" + std::to_string(i) + ")";
    return "";
}
// A bias estimate's layout and values (include/ftmpc.h, ftmpc_bias_estimate) over the vehicles [0, B), against the estimator and the
// disturbance estimate of the same call: empty when acceptable, else the message
std::string bias_problem(const ftmpc_bias_estimate* be, int64_t B, const ftmpc_estimator* es, const ftmpc_disturbance* db,
                                int64_t first = 0) {
    if (!be) return "";
    if (be->struct_size != (int32_t)sizeof(ftmpc_bias_estimate))
        return "ftmpc_bias_estimate.struct_size is " + std::to_string(be->struct_size) + ", this library expects " +
               std::to_string(sizeof(ftmpc_bias_estimate));
    if (!es) return "ftmpc_bias_estimate needs an estimator (ftmpc_estimator): the bias states augment its filter";
    if (db) return "ftmpc_bias_estimate with a disturbance (ftmpc_disturbance) in the same call: 24 filter states are not served";
    for (int k = 0; k < 2; ++k) {
        if (!std::isfinite(be->p0[k]) || be->p0[k] < 0) return "ftmpc_bias_estimate.p0[" + std::to_string(k) + "] is negative or not finite";
        if (!std::isfinite(be->proc_sigma[k]) || be->proc_sigma[k] < 0)
            return "ftmpc_bias_estimate.proc_sigma[" + std::to_string(k) + "] is negative or not finite";
    }
    if (be->cross && !be->bias) return "ftmpc_bias_estimate.cross is given without bias";
    if (be->cross && !es->xhat) return "ftmpc_bias_estimate.cross is given without ftmpc_estimator.xhat";
    if (be->cov && !be->cross) return "ftmpc_bias_estimate.cov is given without cross";
    const double* const arr[3] = {be->bias, be->cross, be->cov};
    const char* const name[3] = {"bias", "cross", "cov"};
    const int64_t width[3] = {6, 72, 21};
    for (int a = 0; a < 3; ++a)
        if (arr[a])
            for (int64_t i = 0; i < B * width[a]; ++i)
                if (!std::isfinite(arr[a][i]))
                    return std::string("ftmpc_bias_estimate.") + name[a] + ": vehicle " + std::to_string(first + i / width[a]) +
                           " has a non-finite entry (" + std::to_string(i % width[a]) + ")";
    if (be->cov)
        for (int64_t b = 0; b < B; ++b)
            for (int i = 0, k = 0; i < 6; k += 6 - i, ++i)
                if (be->cov[b * 21 + k] < 0)
                    return "ftmpc_bias_estimate.cov: vehicle " + std::to_string(first + b) + " has a negative diagonal entry (" + std::to_string(i) + ")";
    return "";
}

// An outage's layout and values (include/ftmpc.h, ftmpc_outage) over the vehicles [0, B), against the estimator and the two estimates of
// the same call: empty when acceptable, else the message, which names the field and, for an array, the first offending vehicle
std::string outage_problem(const ftmpc_outage* og, int64_t B, const ftmpc_estimator* es, const ftmpc_disturbance* db,
                           const ftmpc_bias_estimate* be, int64_t first = 0) {
    if (!og) return "";
    if (og->struct_size != (int32_t)sizeof(ftmpc_outage))
        return "ftmpc_outage.struct_size is " + std::to_string(og->struct_size) + ", this library expects " + std::to_string(sizeof(ftmpc_outage));
    if (og->reserved != 0) return "ftmpc_outage.reserved is " + std::to_string(og->reserved) + ", not 0";
    if (!es) return "ftmpc_outage needs an estimator (ftmpc_estimator): the availability and the gate act on its filter";
    if (db) return "ftmpc_outage with a disturbance (ftmpc_disturbance) in the same call: ftmpc_filter_dist_kernel has no gated form";
    if (be) return "ftmpc_outage with a bias estimate (ftmpc_bias_estimate) in the same call: ftmpc_filter_bias_kernel has no gated form";
    if (!(og->p_loss >= 0.0 && og->p_loss < 1.0)) return "ftmpc_outage.p_loss is outside [0, 1)";
    if (!(og->p_recover > 0.0 && og->p_recover <= 1.0)) return "ftmpc_outage.p_recover is outside (0, 1]";
    for (int k = 0; k < 4; ++k) {
        if (!(og->p_outlier[k] >= 0.0 && og->p_outlier[k] <= 1.0)) return "ftmpc_outage.p_outlier[" + std::to_string(k) + "] is outside [0, 1]";
        if (!std::isfinite(og->outlier_sigma[k]) || og->outlier_sigma[k] < 0)
            return "ftmpc_outage.outlier_sigma[" + std::to_string(k) + "] is negative or not finite";
    }
    if (!std::isfinite(og->gate) || og->gate < 0) return "ftmpc_outage.gate is negative or not finite";
    const int32_t* const arr[3] = {og->state, og->rejected, og->outliers};
    const char* const name[3] = {"state", "rejected", "outliers"};
    const int64_t width[3] = {3, 4, 4};
    for (int a = 0; a < 3; ++a)
        if (arr[a])
            for (int64_t i = 0; i < B * width[a]; ++i)
                if (arr[a][i] < 0)
                    return std::string("ftmpc_outage.") + name[a] + ": vehicle " + std::to_string(first + i / width[a]) +
                           " has a negative entry (" + std::to_string(i % width[a]) + ")";
    return "";
}
// trivial: the loop launches the kernels it launches without the struct
bool outage_trivial(const ftmpc_outage* og) {
    return !og || (og->p_loss == 0 && og->p_outlier[0] == 0 && og->p_outlier[1] == 0 && og->p_outlier[2] == 0 && og->p_outlier[3] == 0 &&
                   og->gate == 0 && !og->window && !og->state && !og->rejected && !og->outliers && !og->avail_hist && !og->outlier_hist &&
                   !og->gate_hist && !og->meas_hist);
}

// An environment's layout and values (include/ftmpc.h, ftmpc_environment) over the vehicles [0, B), against the sensor and the
// disturbance estimate of the same call: empty when acceptable, else the message, which names the field and, for an array, the first
// offending vehicle
std::string environment_problem(const ftmpc_environment* ev, int64_t B, const ftmpc_sensor* se, const ftmpc_disturbance* db,
                                int64_t first = 0) {
    if (!ev) return "";
    if (ev->struct_size != (int32_t)sizeof(ftmpc_environment))
        return "ftmpc_environment.struct_size is " + std::to_string(ev->struct_size) + ", this library expects " +
               std::to_string(sizeof(ftmpc_environment));
    if (ev->reserved != 0) return "ftmpc_environment.reserved is " + std::to_string(ev->reserved) + ", not 0";
    if (ev->step0 < 0) return "ftmpc_environment.step0 is negative";
    if (se && se->step0 != ev->step0)
        return "ftmpc_environment.step0 is " + std::to_string(ev->step0) + ", the sensor's (ftmpc_sensor.step0) is " +
               std::to_string(se->step0) + ": one campaign clock per call";
    for (int a = 0; a < 2; ++a) {
        if (!std::isfinite(ev->sigma[a]) || ev->sigma[a] < 0)
            return "ftmpc_environment.sigma[" + std::to_string(a) + "] is negative or not finite";
        if (ev->sigma[a] > 0 && !(std::isfinite(ev->tau[a]) && ev->tau[a] > 0))
            return "ftmpc_environment.tau[" + std::to_string(a) + "] is not positive and finite (sigma[" + std::to_string(a) + "] > 0)";
    }
    if ((ev->amp_force || ev->amp_torque) && !(std::isfinite(ev->period) && ev->period > 0))
        return "ftmpc_environment.period is not positive and finite (an amplitude is given)";
    if (ev->kick && !ev->window) return "ftmpc_environment.kick without ftmpc_environment.window";
    if (ev->est_err_sq && !db)
        return "ftmpc_environment.est_err_sq needs a disturbance estimate (ftmpc_disturbance) in the same call";
    const double* const arr[6] = {ev->amp_force, ev->amp_torque, ev->phase, ev->kick, ev->state, ev->est_err_sq};
    const char* const name[6] = {"amp_force", "amp_torque", "phase", "kick", "state", "est_err_sq"};
    const int64_t width[6] = {3, 3, 1, 6, 6, 2};
    for (int a = 0; a < 6; ++a)
        if (arr[a])
            for (int64_t i = 0; i < B * width[a]; ++i) {
                if (!std::isfinite(arr[a][i]))
                    return std::string("ftmpc_environment.") + name[a] + ": vehicle " + std::to_string(first + i / width[a]) +
                           " has a non-finite entry (" + std::to_string(i % width[a]) + ")";
                if (a == 5 && arr[a][i] < 0)
                    return std::string("ftmpc_environment.est_err_sq: vehicle ") + std::to_string(first + i / 2) + " has a negative entry (" +
                           std::to_string(i % 2) + ")";
            }
    return "";
}
// trivial: the loop launches the kernels it launches without the struct
bool environment_trivial(const ftmpc_environment* ev) {
    return !ev || (ev->sigma[0] == 0 && ev->sigma[1] == 0 && !ev->amp_force && !ev->amp_torque && !ev->phase && !ev->kick && !ev->window &&
                   !ev->state && !ev->wrench_hist && !ev->est_err_sq);
}

// trivial: the loop launches the kernels it launches without the struct
bool isolation_trivial(const ftmpc_isolation* is) {
    return !is || (is->consist == 0 && is->persist == 1 && is->revise == 0 && !is->lead && !is->voided && !is->revised && !is->fit_hist);
}
// An isolation's layout and values (include/ftmpc.h, ftmpc_isolation) over the vehicles [0, B), against the diagnosis of the same
// call: empty when acceptable, else the message, which names the field and, for an array, the first offending vehicle
std::string isolation_problem(const ftmpc_isolation* is, int64_t B, int NT, const ftmpc_diagnosis* dg, int64_t first = 0,
                              bool reinstating = false) {
    if (!is) return "";
    if (is->struct_size != (int32_t)sizeof(ftmpc_isolation))
        return "ftmpc_isolation.struct_size is " + std::to_string(is->struct_size) + ", this library expects " +
               std::to_string(sizeof(ftmpc_isolation));
    if (is->reserved != 0) return "ftmpc_isolation.reserved is " + std::to_string(is->reserved) + ", not 0";
    if (!std::isfinite(is->consist) || is->consist < 0) return "ftmpc_isolation.consist is negative or not finite";
    if (is->persist < 1) return "ftmpc_isolation.persist is " + std::to_string(is->persist) + ", not >= 1";
    if (is->revise != 0 && is->revise != 1) return "ftmpc_isolation.revise is " + std::to_string(is->revise) + ", not 0 or 1";
    if (!isolation_trivial(is) && !dg)
        return "ftmpc_isolation: consist, persist, revise or an array is set, but the call has no diagnosis (ftmpc_diagnosis) whose "
               "rule they could change";
    if (is->lead && !dg->state) return "ftmpc_isolation.lead without ftmpc_diagnosis.state";
    if (is->lead) {
        // (under a reinstating probe the leader may be H + i, "thruster i is healthy")
        const int64_t H = (int64_t)NT * dg->n_levels + (reinstating ? NT : 0);
        for (int64_t b = 0; b < B; ++b) {
            if (is->lead[b * 2] < -1 || is->lead[b * 2] >= H)
                return "ftmpc_isolation.lead: vehicle " + std::to_string(first + b) + " has a leader outside [-1, NT * n_levels)";
            if (is->lead[b * 2 + 1] < 0) return "ftmpc_isolation.lead: vehicle " + std::to_string(first + b) + " has a negative run";
        }
    }
    const int32_t* const arr[2] = {is->voided, is->revised};
    const char* const name[2] = {"voided", "revised"};
    for (int a = 0; a < 2; ++a)
        if (arr[a])
            for (int64_t b = 0; b < B; ++b)
                if (arr[a][b] < 0)
                    return std::string("ftmpc_isolation.") + name[a] + ": vehicle " + std::to_string(first + b) + " has a negative entry";
    return "";
}

// a probe that replaces the phase-0 diagnosis kernel and widens the detect_level and lead checks
bool probe_reinstates(const ftmpc_probe* pb) {
    return pb && pb->struct_size == (int32_t)sizeof(ftmpc_probe) && pb->reinstate == 1;
}
// A probe's layout and values (include/ftmpc.h, ftmpc_probe) over the vehicles [0, B), against the diagnosis of the same call: empty
// when acceptable, else the message, which names the field and, for an array, the first offending vehicle
std::string probe_problem(const ftmpc_probe* pb, int64_t B, int NT, const ftmpc_diagnosis* dg, int64_t first = 0) {
    if (!pb) return "";
    if (pb->struct_size != (int32_t)sizeof(ftmpc_probe))
        return "ftmpc_probe.struct_size is " + std::to_string(pb->struct_size) + ", this library expects " + std::to_string(sizeof(ftmpc_probe));
    if (pb->reserved != 0) return "ftmpc_probe.reserved is " + std::to_string(pb->reserved) + ", not 0";
    if (!dg) return "ftmpc_probe: the call has no diagnosis (ftmpc_diagnosis) whose pattern and detection list the probe reads";
    if (!std::isfinite(pb->amp) || !(pb->amp > 0)) return "ftmpc_probe.amp is not finite and > 0";
    if (!(pb->quiet >= 0 && pb->quiet < pb->amp)) return "ftmpc_probe.quiet is outside [0, amp)";
    if (pb->idle_steps < 1) return "ftmpc_probe.idle_steps is " + std::to_string(pb->idle_steps) + ", not >= 1";
    if (pb->max_pulses < 0) return "ftmpc_probe.max_pulses is negative";
    if (pb->reinstate != 0 && pb->reinstate != 1) return "ftmpc_probe.reinstate is " + std::to_string(pb->reinstate) + ", not 0 or 1";
    if (pb->reinstate == 1 && (!std::isfinite(pb->restore_ub) || !(pb->restore_ub > 0)))
        return "ftmpc_probe.restore_ub is not finite and > 0 (reinstate = 1)";
    if (pb->pacc && !dg->state) return "ftmpc_probe.pacc without ftmpc_diagnosis.state";
    if (pb->health && !dg->state) return "ftmpc_probe.health without ftmpc_diagnosis.state";
    const int32_t* const iarr[3] = {pb->idle, pb->pulses, pb->reinstated};
    const char* const iname[3] = {"idle", "pulses", "reinstated"};
    const int64_t iwidth[3] = {NT, NT, 1};
    for (int a = 0; a < 3; ++a)
        if (iarr[a])
            for (int64_t i = 0; i < B * iwidth[a]; ++i)
                if (iarr[a][i] < 0)
                    return std::string("ftmpc_probe.") + iname[a] + ": vehicle " + std::to_string(first + i / iwidth[a]) + " has a negative entry";
    const double* const darr[3] = {pb->impulse, pb->pacc, pb->health};
    const char* const dname[3] = {"impulse", "pacc", "health"};
    const int64_t dwidth[3] = {1, NT, NT};
    for (int a = 0; a < 3; ++a)
        if (darr[a])
            for (int64_t i = 0; i < B * dwidth[a]; ++i)
                if (!std::isfinite(darr[a][i]) || darr[a][i] < 0)
                    return std::string("ftmpc_probe.") + dname[a] + ": vehicle " + std::to_string(first + i / dwidth[a]) +
                           " has a negative or non-finite entry";
    return "";
}

int check_estimator(ftmpc_handle* h, int64_t B, const ftmpc_estimator* es) {
    const std::string msg = estimator_problem(es, B);
    return msg.empty() ? FTMPC_OK : fail(h, FTMPC_ERR_ARG, msg);
}

// A diagnosis' layout and values (include/ftmpc.h, ftmpc_diagnosis) over the vehicles [0, B), against the estimator, the schedule and
// the sensor of the same call: empty when acceptable, else the message, which names the field and, for an array, the first offending
// vehicle (first: number of vehicle 0 in the caller's batch)
std::string diagnosis_problem(const ftmpc_diagnosis* dg, int64_t B, int NT, const ftmpc_estimator* es, const ftmpc_fault_schedule* fs,
                                     const ftmpc_sensor* se, int64_t first = 0, bool reinstating = false) {
    if (!dg) return "";
    if (dg->struct_size != (int32_t)sizeof(ftmpc_diagnosis))
        return "ftmpc_diagnosis.struct_size is " + std::to_string(dg->struct_size) + ", this library expects " +
               std::to_string(sizeof(ftmpc_diagnosis));
    if (dg->every < 1) return "ftmpc_diagnosis.every is " + std::to_string(dg->every) + ", below 1";
    if (es && es->every != dg->every)
        return "ftmpc_diagnosis.every is " + std::to_string(dg->every) + ", the estimator's every is " + std::to_string(es->every);
    if (dg->n_levels < 1 || dg->n_levels > 4) return "ftmpc_diagnosis.n_levels is " + std::to_string(dg->n_levels) + ", outside [1, 4]";
    if (dg->max_detect < 1 || dg->max_detect > FTMPC_MAX_FAULT_EVENTS)
        return "ftmpc_diagnosis.max_detect is " + std::to_string(dg->max_detect) + ", outside [1, FTMPC_MAX_FAULT_EVENTS]";
    for (int l = 0; l < dg->n_levels; ++l)
        if (!std::isfinite(dg->levels[l]) || dg->levels[l] < 0 || (l > 0 && !(dg->levels[l] > dg->levels[l - 1])))
            return "ftmpc_diagnosis.levels[" + std::to_string(l) + "] is negative, not finite or not above the level before";
    for (int k = 0; k < 2; ++k) {
        if (!std::isfinite(dg->resid_sigma[k]) || !(dg->resid_sigma[k] > 0))
            return "ftmpc_diagnosis.resid_sigma[" + std::to_string(k) + "] is not finite and > 0";
        if (!std::isfinite(dg->drift_sigma[k]) || dg->drift_sigma[k] < 0)
            return "ftmpc_diagnosis.drift_sigma[" + std::to_string(k) + "] is negative or not finite";
    }
    if (!std::isfinite(dg->threshold) || !(dg->threshold > 0)) return "ftmpc_diagnosis.threshold is not finite and > 0";
    if (dg->llr && !dg->state) return "ftmpc_diagnosis.llr is given without state";
    if (!dg->state && dg->detect_step) return "ftmpc_diagnosis.detect_step is given without state";
    if (!dg->state && dg->detect_thruster) return "ftmpc_diagnosis.detect_thruster is given without state";
    if (!dg->state && dg->detect_level) return "ftmpc_diagnosis.detect_level is given without state";
    if (dg->state) {
        if (!dg->detect_step) return "ftmpc_diagnosis.detect_step is required with state";
        if (!dg->detect_thruster) return "ftmpc_diagnosis.detect_thruster is required with state";
        if (!dg->detect_level) return "ftmpc_diagnosis.detect_level is required with state";
        const int64_t w = 14 + NT, H = (int64_t)NT * dg->n_levels, K = dg->max_detect;
        for (int64_t b = 0; b < B; ++b) {
            const double* st = dg->state + b * w;
            for (int64_t k = 0; k < w; ++k)
                if (!std::isfinite(st[k]))
                    return "ftmpc_diagnosis.state: vehicle " + std::to_string(first + b) + " has a non-finite entry (" + std::to_string(k) + ")";
            if (st[13] < 0) return "ftmpc_diagnosis.state: vehicle " + std::to_string(first + b) + " has n < 0";
            if (dg->llr)
                for (int64_t k = 0; k < H; ++k)
                    if (!std::isfinite(dg->llr[b * H + k]))
                        return "ftmpc_diagnosis.llr: vehicle " + std::to_string(first + b) + " has a non-finite entry (" + std::to_string(k) + ")";
            bool unused = false;
            for (int64_t k = 0; k < K; ++k) {
                const int32_t ds = dg->detect_step[b * K + k], dt = dg->detect_thruster[b * K + k], dl = dg->detect_level[b * K + k];
                if (ds == -1) {
                    unused = true;
                    continue;
                }
                if (ds < -1) return "ftmpc_diagnosis.detect_step: vehicle " + std::to_string(first + b) + " has an entry below -1";
                if (unused) return "ftmpc_diagnosis.detect_step: vehicle " + std::to_string(first + b) + " has a used slot after an unused one";
                if (dt < 0 || dt >= NT)
                    return "ftmpc_diagnosis.detect_thruster: vehicle " + std::to_string(first + b) + " has an entry outside [0, NT)";
                // (under a reinstating probe an entry at n_levels is a reinstatement)
                if (dl < 0 || dl >= dg->n_levels + (reinstating ? 1 : 0))
                    return "ftmpc_diagnosis.detect_level: vehicle " + std::to_string(first + b) + " has an entry outside [0, n_levels)";
            }
        }
    }
    if (fs && fs->n_events > 0 && fs->detect)
        return "ftmpc_diagnosis: ftmpc_fault_schedule.detect must be NULL (the schedule moves the plant only, the diagnosis detects)";
    if (se && se->predict == 1 && !es)
        return "ftmpc_diagnosis: ftmpc_sensor.predict = 1 needs an estimator (the sense kernel would predict with the pattern before the diagnosis)";
    return "";
}

// What the wrench form adds to a diagnosis' refusals: the schedule of such a call moves the plant only, so it carries no hull tables,
// and a handed no_hull_step entry is -1 or a step (first: number of vehicle 0 in the caller's batch)
std::string wrench_diagnosis_problem(const ftmpc_fault_schedule* fs, const int32_t* no_hull_step, int64_t B, int64_t first = 0) {
    if (fs && fs->struct_size == (int32_t)sizeof(ftmpc_fault_schedule)) {
        if (fs->hull_set) return "ftmpc_diagnosis: ftmpc_fault_schedule.hull_set must be NULL (the schedule moves the plant only, the diagnosis rebuilds the offsets)";
        if (fs->hull_b) return "ftmpc_diagnosis: ftmpc_fault_schedule.hull_b must be NULL (the schedule moves the plant only, the diagnosis rebuilds the offsets)";
    }
    if (no_hull_step)
        for (int64_t b = 0; b < B; ++b)
            if (no_hull_step[b] < -1) return "no_hull_step: vehicle " + std::to_string(first + b) + " has an entry below -1";
    return "";
}

// An outcomes struct's layout and values (include/ftmpc.h, ftmpc_outcomes); wrench: the form with an allocation
int check_outcomes(ftmpc_handle* h, int64_t B, const ftmpc_outcomes* oc, bool wrench) {
    if (!oc) return FTMPC_OK;
    if (oc->struct_size != (int32_t)sizeof(ftmpc_outcomes))
        return fail(h, FTMPC_ERR_ARG, "ftmpc_outcomes.struct_size is " + std::to_string(oc->struct_size) + ", this library expects " +
                                          std::to_string(sizeof(ftmpc_outcomes)));
    if (oc->index0 < 0) return fail(h, FTMPC_ERR_ARG, "ftmpc_outcomes.index0 is negative");
    if (oc->index_total == 0 && oc->index0 != 0)
        return fail(h, FTMPC_ERR_ARG, "ftmpc_outcomes.index_total = 0 (the call is the campaign) needs index0 = 0");
    if (oc->index_total != 0 && (oc->index_total < 0 || oc->index0 > oc->index_total - B))
        return fail(h, FTMPC_ERR_ARG, "ftmpc_outcomes.index_total: index0 + B = " + std::to_string(oc->index0) + " + " + std::to_string(B) +
                                          " exceeds index_total = " + std::to_string(oc->index_total));
    if (oc->settle_step) {
        const double tol[3] = {oc->tol_pos, oc->tol_vel, oc->tol_rate};
        const char* name[3] = {"tol_pos", "tol_vel", "tol_rate"};
        for (int i = 0; i < 3; ++i)
            if (!(tol[i] > 0.0) || !std::isfinite(tol[i]))
                return fail(h, FTMPC_ERR_ARG, std::string("ftmpc_outcomes.") + name[i] + " must be positive and finite when settle_step is asked for");
    }
    if (oc->tset_step && (h->cfg.term_rows < 1 || h->cfg.term_rows > FTMPC_MAX_TERM_ROWS))
        return fail(h, FTMPC_ERR_ARG, "ftmpc_outcomes.tset_step needs the terminal rows of the handle's config (term_rows in 1..80)");
    if (oc->alloc_failed && !wrench)
        return fail(h, FTMPC_ERR_ARG, "ftmpc_outcomes.alloc_failed: the thruster form has no allocation (use ftmpc_simulate_wrench_outcomes_batch)");
    return FTMPC_OK;
}

// A fault schedule's layout and values (include/ftmpc.h, ftmpc_fault_schedule).  wrench: the wrench form, whose call has n_sets hull
// tables of hull_rows rows and its own hull_set (call_set) or not.
int check_schedule(ftmpc_handle* h, int64_t B, const ftmpc_fault_schedule* fs, bool wrench, int32_t n_sets, bool call_set) {
    if (!fs) return FTMPC_OK;
    if (fs->struct_size != (int32_t)sizeof(ftmpc_fault_schedule)) return fail(h, FTMPC_ERR_ARG, "ftmpc_fault_schedule: bad struct_size");
    if (fs->n_events < 0 || fs->n_events > FTMPC_MAX_FAULT_EVENTS)
        return fail(h, FTMPC_ERR_ARG, "ftmpc_fault_schedule: n_events outside [0, FTMPC_MAX_FAULT_EVENTS]");
    const int E = fs->n_events, NT = h->cfg.NT;
    if (E == 0) return FTMPC_OK;
    if (!fs->onset || !fs->ub || !fs->stuck) return fail(h, FTMPC_ERR_ARG, "ftmpc_fault_schedule: null onset / ub / stuck");
    if (wrench && !fs->hull_b) return fail(h, FTMPC_ERR_ARG, "ftmpc_fault_schedule: the wrench form needs hull_b");
    if (wrench && fs->hull_set && !call_set)
        return fail(h, FTMPC_ERR_ARG, "ftmpc_fault_schedule: per-event hull_set, but the call's hull_set is NULL (one table)");
    if (wrench && !fs->hull_set && call_set)
        return fail(h, FTMPC_ERR_ARG, "ftmpc_fault_schedule: the call has a hull_set per instance, the schedule needs one per event");
    for (int64_t b = 0; b < B; ++b) {
        int32_t pon = -1, pde = -1;
        bool unused = false;
        for (int e = 0; e < E; ++e) {
            const int64_t i = b * E + e;
            const int32_t on = fs->onset[i];
            if (on == -1) {
                unused = true;
                continue;
            }
            if (on < -1) return fail(h, FTMPC_ERR_ARG, "ftmpc_fault_schedule: onset below -1");
            if (unused) return fail(h, FTMPC_ERR_ARG, "ftmpc_fault_schedule: a used slot after an unused one");
            const int32_t de = fs->detect ? fs->detect[i] : on;
            if (de < on) return fail(h, FTMPC_ERR_ARG, "ftmpc_fault_schedule: detect < onset");
            if (on < pon || de < pde) return fail(h, FTMPC_ERR_ARG, "ftmpc_fault_schedule: slots not sorted by onset and detect");
            pon = on;
            pde = de;
            for (int k = 0; k < NT; ++k) {
                const double u = fs->ub[i * NT + k], st = fs->stuck[i * NT + k];
                if (!std::isfinite(u) || u < 0.0) return fail(h, FTMPC_ERR_ARG, "ftmpc_fault_schedule: negative or non-finite ub");
                if (!std::isfinite(st)) return fail(h, FTMPC_ERR_ARG, "ftmpc_fault_schedule: non-finite stuck");
            }
            if (wrench && fs->hull_set && (fs->hull_set[i] < 0 || fs->hull_set[i] >= n_sets))
                return fail(h, FTMPC_ERR_ARG, "ftmpc_fault_schedule: hull_set outside [0, n_sets)");
        }
    }
    return FTMPC_OK;
}

// the ABI guard of a bias estimate, before the handle is looked at (so that it needs no device): the message goes to the handle's
// error, or to the one ftmpc_last_error(NULL) returns
int check_bias_size(ftmpc_handle* h, const ftmpc_bias_estimate* be) {
    if (be && be->struct_size != (int32_t)sizeof(ftmpc_bias_estimate)) return fail(h, FTMPC_ERR_ARG, bias_problem(be, 0, nullptr, nullptr));
    return FTMPC_OK;
}

// ---- the stage structs: one per feature.  Each owns the feature's device buffers (freed by scope on every way out of simulate_core),
// its host staging vectors (which live until the final synchronise: asynchronous copies read and write them) and its kernel parameter
// block.  stage: allocate, convert, upload and fill the block, before step 0; fetch: the asynchronous read-backs after step T - 1;
// unpack: the host conversions after the synchronise.  Pointers from one feature's block into another feature's buffers are not set
// here but in simulate_core ("the wiring").

// what every stage operation needs of the call
struct Loop {
    ftmpc_handle* h;
    hipStream_t s;
    int64_t B;
    int32_t T;
    int N, NT;
    int64_t index0, index_total;      // the slice of the campaign (ftmpc_outcomes): what the random streams are keyed by
};

#define LOOP_TRY(expr)                           \
    do {                                         \
        const int rc__ = (expr);                 \
        if (rc__ != FTMPC_OK) return rc__;       \
    } while (0)

template <typename V>
int dev_alloc(const Loop& q, DevBuf<V>& d, size_t n) {
    HIP_TRY(q.h, hipMalloc(&d.p, n * sizeof(V)));
    return FTMPC_OK;
}
template <typename V>
int dev_fill(const Loop& q, V* dst, int byte, size_t n) {
    HIP_TRY(q.h, hipMemsetAsync(dst, byte, n * sizeof(V), q.s));
    return FTMPC_OK;
}
template <typename V>
int dev_put(const Loop& q, V* dst, const V* src, size_t n) {
    HIP_TRY(q.h, hipMemcpyAsync(dst, src, n * sizeof(V), hipMemcpyHostToDevice, q.s));
    return FTMPC_OK;
}
template <typename V>
int dev_get(const Loop& q, V* dst, const V* src, size_t n) {
    HIP_TRY(q.h, hipMemcpyAsync(dst, src, n * sizeof(V), hipMemcpyDeviceToHost, q.s));
    return FTMPC_OK;
}
// a history [T][...] the caller asked for (host != null): room for it before the loop, the read-back after it
template <typename V>
int hist_alloc(const Loop& q, DevBuf<V>& d, const V* host, size_t n) {
    return host ? dev_alloc(q, d, n) : FTMPC_OK;
}
template <typename V>
int hist_get(const Loop& q, V* host, const DevBuf<V>& d, size_t n) {
    return host ? dev_get(q, host, d.p, n) : FTMPC_OK;
}

// The call's own arrays: the reference trajectories (without mission tables), the thruster form's warm start, the histories and the
// per-step counts; x, ub and stuck go into the handle's buffers
struct RunStage {
    DevBuf<double> d_xr, d_ur, d_warmB, d_hist, d_xhist;
    DevBuf<int32_t> d_bad, d_abad;

    int stage(const Loop& q, const LoopCall& c, bool windows, int64_t ncol) {
        const size_t T = (size_t)q.T, B = (size_t)q.B;
        if (!windows) LOOP_TRY(dev_alloc(q, d_xr, (size_t)ncol * 9));
        if (c.uref_traj) LOOP_TRY(dev_alloc(q, d_ur, (size_t)ncol * 6));
        if (!c.wrench) LOOP_TRY(dev_alloc(q, d_warmB, B * q.N * q.NT));
        if (c.wrench && c.alloc_failed) {
            LOOP_TRY(dev_alloc(q, d_abad, T));
            LOOP_TRY(dev_fill(q, d_abad.p, 0, T));
        }
        LOOP_TRY(hist_alloc(q, d_hist, c.u_hist, T * B * q.NT));
        LOOP_TRY(hist_alloc(q, d_xhist, c.x_hist, T * B * 13));
        LOOP_TRY(dev_alloc(q, d_bad, T));
        LOOP_TRY(dev_fill(q, d_bad.p, 0, T));
        if (!windows) LOOP_TRY(dev_put(q, d_xr.p, c.xref_traj, (size_t)ncol * 9));
        if (c.uref_traj) LOOP_TRY(dev_put(q, d_ur.p, c.uref_traj, (size_t)ncol * 6));
        return stage_inputs(q.h, q.B, c.x, c.ub, c.stuck);
    }
    int fetch(const Loop& q, const LoopCall& c) {
        const size_t T = (size_t)q.T, B = (size_t)q.B;
        if (c.wrench && c.out_hull_b) LOOP_TRY(dev_get(q, c.out_hull_b, q.h->d_hullb.p, B * c.hull_rows));
        LOOP_TRY(hist_get(q, c.u_hist, d_hist, T * B * q.NT));
        LOOP_TRY(hist_get(q, c.x_hist, d_xhist, T * B * 13));
        LOOP_TRY(hist_get(q, c.not_converged, d_bad, T));
        if (d_abad) LOOP_TRY(dev_get(q, c.alloc_failed, d_abad.p, T));
        return FTMPC_OK;
    }
};

// Plant model (checked by the entry): the arrays that are given, component-major [k][B] (the layout of ftmpc::PlantVar), 1 / m_b and
// J_b^-1 computed here, once per call
struct PlantStage {
    bool var = false;      // some array is given: the plant's step is ftmpc_plant_step_var_kernel's (or the actuator's)
    DevBuf<double> d_im, d_J, d_D, d_f, d_t;
    std::vector<double> h_im, h_J, h_D, h_f, h_t;
    ftmpc::PlantVar pv{};

    int stage(const Loop& q, const ftmpc_plant_model* pm) {
        var = pm && (pm->mass || pm->J || pm->D || pm->force || pm->torque);
        if (!var) return FTMPC_OK;
        const int64_t B = q.B;
        auto packed = [&](const double* src, int64_t K, std::vector<double>& v) {
            if (!src) return;
            v.resize((size_t)(B * K));
            ftmpc::pack_kb(src, B, K, v.data());
        };
        auto upload = [&](DevBuf<double>& d, const std::vector<double>& v) -> int {
            if (v.empty()) return FTMPC_OK;
            LOOP_TRY(dev_alloc(q, d, v.size()));
            return dev_put(q, d.p, v.data(), v.size());
        };
        try {
            if (pm->mass) {
                h_im.resize((size_t)B);
                for (int64_t b = 0; b < B; ++b) h_im[b] = 1.0 / pm->mass[b];
            }
            if (pm->J) {      // J with its inverse appended: [18][B]
                h_J.resize((size_t)B * 18);
                for (int64_t b = 0; b < B; ++b) {
                    const double* J = pm->J + b * 9;
                    const double c00 = J[4] * J[8] - J[5] * J[7], c01 = J[5] * J[6] - J[3] * J[8], c02 = J[3] * J[7] - J[4] * J[6];
                    const double idet = 1.0 / (J[0] * c00 + J[1] * c01 + J[2] * c02);
                    const double inv[9] = {c00 * idet, (J[2] * J[7] - J[1] * J[8]) * idet, (J[1] * J[5] - J[2] * J[4]) * idet,
                                           c01 * idet, (J[0] * J[8] - J[2] * J[6]) * idet, (J[2] * J[3] - J[0] * J[5]) * idet,
                                           c02 * idet, (J[1] * J[6] - J[0] * J[7]) * idet, (J[0] * J[4] - J[1] * J[3]) * idet};
                    for (int k = 0; k < 9; ++k) {
                        h_J[(size_t)k * B + b] = J[k];
                        h_J[(size_t)(9 + k) * B + b] = inv[k];
                    }
                }
            }
            packed(pm->D, 6 * (int64_t)q.NT, h_D);
            packed(pm->force, 3, h_f);
            packed(pm->torque, 3, h_t);
        } catch (const std::bad_alloc&) {
            return fail(q.h, FTMPC_ERR_ALLOC, "out of host memory for the plant model's staging arrays");
        }
        LOOP_TRY(upload(d_im, h_im));
        LOOP_TRY(upload(d_J, h_J));
        LOOP_TRY(upload(d_D, h_D));
        LOOP_TRY(upload(d_f, h_f));
        LOOP_TRY(upload(d_t, h_t));
        pv.inv_mass = d_im;
        pv.J = d_J;
        pv.D = d_D;
        pv.force = d_f;
        pv.torque = d_t;
        return FTMPC_OK;
    }
};

// Actuator (checked by the entry): not trivial, the plant's step is ftmpc_plant_step_act_kernel's.  The four lag constants are computed
// here, once per call; the valve states are staged component-major [NT][B], delivered and pulses start at zero
struct ActuatorStage {
    bool on = false;
    DevBuf<double> d_val, d_del, d_app;
    DevBuf<int32_t> d_pul, d_tick;
    std::vector<double> h_val;
    ftmpc::ActParams ap{};

    int stage(const Loop& q, const ftmpc_actuator* ac) {
        on = !actuator_trivial(ac);
        if (!on) return FTMPC_OK;
        const int S = ac->substeps > 0 ? ac->substeps : 1;
        const double hs = q.h->cfg.dt / S;
        ap.pwm = ac->mode == 1;
        ap.substeps = S;
        ap.min_on = ac->min_on;
        ap.align = ac->align;
        if (ac->tau_on > 0) {
            ap.E_on = std::exp(-hs / ac->tau_on);
            ap.K_on = -std::expm1(-hs / ac->tau_on) * ac->tau_on / hs;
        }
        if (ac->tau_off > 0) {
            ap.E_off = std::exp(-hs / ac->tau_off);
            ap.K_off = -std::expm1(-hs / ac->tau_off) * ac->tau_off / hs;
        }
        const size_t B = (size_t)q.B, nv = B * q.NT;
        LOOP_TRY(dev_alloc(q, d_val, nv));
        LOOP_TRY(dev_alloc(q, d_del, B));
        LOOP_TRY(dev_alloc(q, d_pul, B));
        LOOP_TRY(dev_fill(q, d_del.p, 0, B));
        LOOP_TRY(dev_fill(q, d_pul.p, 0, B));
        if (ac->state) {
            try {
                h_val.resize(nv);
            } catch (const std::bad_alloc&) {
                return fail(q.h, FTMPC_ERR_ALLOC, "out of host memory for the actuator's staging array");
            }
            ftmpc::pack_kb(ac->state, q.B, q.NT, h_val.data());
            LOOP_TRY(dev_put(q, d_val.p, h_val.data(), nv));
        } else {
            LOOP_TRY(dev_fill(q, d_val.p, 0, nv));
        }
        LOOP_TRY(hist_alloc(q, d_app, ac->applied_hist, q.T * nv));
        LOOP_TRY(hist_alloc(q, d_tick, ac->ticks_hist, q.T * nv));
        ap.state = d_val;
        ap.delivered = d_del;
        ap.pulses = d_pul;
        ap.applied_hist = d_app;
        ap.ticks_hist = d_tick;
        return FTMPC_OK;
    }
    int fetch(const Loop& q, const ftmpc_actuator* ac) {
        if (!on) return FTMPC_OK;
        const size_t B = (size_t)q.B, nv = B * q.NT;
        LOOP_TRY(hist_get(q, ac->delivered, d_del, B));
        LOOP_TRY(hist_get(q, ac->pulses, d_pul, B));
        LOOP_TRY(hist_get(q, ac->applied_hist, d_app, q.T * nv));
        LOOP_TRY(hist_get(q, ac->ticks_hist, d_tick, q.T * nv));
        if (ac->state) LOOP_TRY(dev_get(q, h_val.data(), d_val.p, nv));
        return FTMPC_OK;
    }
    void unpack(const Loop& q, const ftmpc_actuator* ac) {
        if (on && ac->state) ftmpc::unpack_kb(h_val.data(), q.B, q.NT, ac->state);
    }
};

// Sensor (checked by the entry) and command ring: the truth lives in d_xtrue and ftmpc_sense_kernel writes h->d_x0 before every solve;
// lat commands wait in the ring d_ring ([lat + 1][B][NT]).  An estimator or a diagnosis takes the same truth-buffer path even when the
// sensor is trivial (on: one of the three)
struct SensorStage {
    bool on = false;
    int lat = 0;
    DevBuf<double> d_xtrue, d_ring, d_bias, d_mhist, d_phist;
    std::vector<double> h_ring;
    ftmpc::SenseParams sn{};

    // pending [B][lat][NT] <-> slots [lat][B][NT]
    void ring_copy(const Loop& q, const ftmpc_sensor* se, bool in) {
        const size_t nu = (size_t)q.B * q.NT;
        for (int64_t b = 0; b < q.B; ++b)
            for (int j = 0; j < lat; ++j)
                for (int i = 0; i < q.NT; ++i) {
                    double& host = se->pending[(b * lat + j) * q.NT + i];
                    double& slot = h_ring[(size_t)j * nu + b * q.NT + i];
                    if (in) slot = host;
                    else host = slot;
                }
    }
    int stage(const Loop& q, const ftmpc_sensor* se, bool sense) {
        on = sense;
        if (!on) return FTMPC_OK;
        lat = se->latency;
        const size_t T = (size_t)q.T, B = (size_t)q.B, nu = B * q.NT;
        LOOP_TRY(dev_alloc(q, d_xtrue, B * 13));
        HIP_TRY(q.h, hipMemcpyAsync(d_xtrue, q.h->d_x0, B * 13 * sizeof(double), hipMemcpyDeviceToDevice, q.s));
        if (lat > 0) {      // slots 0 .. lat-1: the pending commands, oldest first
            LOOP_TRY(dev_alloc(q, d_ring, (size_t)(lat + 1) * nu));
            if (se->pending) {
                try {
                    h_ring.resize((size_t)lat * nu);
                } catch (const std::bad_alloc&) {
                    return fail(q.h, FTMPC_ERR_ALLOC, "out of host memory for the sensor's staging array");
                }
                ring_copy(q, se, true);
                LOOP_TRY(dev_put(q, d_ring.p, h_ring.data(), (size_t)lat * nu));
            } else {
                LOOP_TRY(dev_fill(q, d_ring.p, 0, (size_t)lat * nu));
            }
        }
        if (se->bias) {
            LOOP_TRY(dev_alloc(q, d_bias, B * 12));
            LOOP_TRY(dev_put(q, d_bias.p, se->bias, B * 12));
        }
        LOOP_TRY(hist_alloc(q, d_mhist, se->meas_hist, T * B * 13));
        LOOP_TRY(hist_alloc(q, d_phist, se->pred_hist, T * B * 13));
        sn.B = q.B;
        sn.x = d_xtrue;
        sn.y = q.h->d_x0;
        sn.ub = q.h->d_ub;
        sn.stuck = q.h->d_stuck;
        sn.ring = d_ring;
        sn.nslots = lat + 1;
        sn.latency = lat;
        sn.predict = se->predict;
        for (int i = 0; i < 4; ++i) sn.sigma[i] = se->sigma[i];
        sn.bias = d_bias;
        sn.seed = se->seed;
        sn.index0 = q.index0;
        sn.index_total = q.index_total;
        sn.meas_hist = d_mhist;
        sn.pred_hist = d_phist;
        return FTMPC_OK;
    }
    int fetch(const Loop& q, const ftmpc_sensor* se) {
        if (!on) return FTMPC_OK;
        const size_t T = (size_t)q.T, B = (size_t)q.B, nu = B * q.NT;
        LOOP_TRY(hist_get(q, se->meas_hist, d_mhist, T * B * 13));
        LOOP_TRY(hist_get(q, se->pred_hist, d_phist, T * B * 13));
        if (se->pending)      // c_T .. c_{T+lat-1}: the slots from T mod (lat + 1) on, oldest first
            for (int j = 0; j < lat; ++j)
                LOOP_TRY(dev_get(q, h_ring.data() + (size_t)j * nu, d_ring + (size_t)((q.T + j) % (lat + 1)) * nu, nu));
        return FTMPC_OK;
    }
    void unpack(const Loop& q, const ftmpc_sensor* se) {
        if (on && se->pending) ring_copy(q, se, false);
    }
};

// Filter (the estimator, checked by the entry): the mean [B][13] and the packed covariance, component-major [78][B], diag(p0^2) when
// none is handed over; err_sq [B][4] starts at zero
struct FilterStage {
    bool on = false;
    DevBuf<double> d_xhat, d_cov, d_ehist, d_esq;
    std::vector<double> h_cov;
    ftmpc::FilterParams fp{};

    int stage(const Loop& q, const ftmpc_estimator* es, const ftmpc_bias_estimate* be, const ftmpc_sensor* se) {
        on = es != nullptr;
        if (!on) return FTMPC_OK;
        const int64_t B = q.B;
        const size_t nc = (size_t)B * 78;
        try {
            h_cov.assign(nc, 0.0);
        } catch (const std::bad_alloc&) {
            return fail(q.h, FTMPC_ERR_ALLOC, "out of host memory for the estimator's staging array");
        }
        if (es->cov) {
            ftmpc::pack_kb(es->cov, B, 78, h_cov.data());
        } else {
            for (int i = 0, k = 0; i < 12; k += 12 - i, ++i) std::fill(h_cov.begin() + (size_t)k * B, h_cov.begin() + (size_t)(k + 1) * B, es->p0[i / 3] * es->p0[i / 3]);
        }
        if (be && !be->cross)     // a bias estimate without handed pieces: P_mm = P_xx + HB diag(p0_b^2) HB' (see BiasStage)
            for (int i = 0, k = 0; i < 12; k += 12 - i, ++i)
                if ((i >= 3 && i < 6) || i >= 9)
                    for (int64_t b = 0; b < B; ++b) h_cov[(size_t)k * B + b] += be->p0[i >= 9] * be->p0[i >= 9];
        LOOP_TRY(dev_alloc(q, d_cov, nc));
        LOOP_TRY(dev_put(q, d_cov.p, h_cov.data(), nc));
        LOOP_TRY(dev_alloc(q, d_xhat, (size_t)B * 13));
        if (es->xhat) LOOP_TRY(dev_put(q, d_xhat.p, (const double*)es->xhat, (size_t)B * 13));
        LOOP_TRY(hist_alloc(q, d_ehist, es->est_hist, (size_t)q.T * B * 13));
        if (es->err_sq) {
            LOOP_TRY(dev_alloc(q, d_esq, (size_t)B * 4));
            LOOP_TRY(dev_fill(q, d_esq.p, 0, (size_t)B * 4));
        }
        fp.B = B;
        fp.latency = se->latency;
        fp.predict = se->predict;
        fp.nslots = se->latency + 1;
        fp.x0 = q.h->d_x0;
        fp.xhat = d_xhat;
        fp.cov = d_cov;
        fp.ub = q.h->d_ub;
        fp.stuck = q.h->d_stuck;
        for (int i = 0; i < 4; ++i) {
            fp.rsq[i] = es->meas_sigma[i] * es->meas_sigma[i];
            fp.qsq[i] = es->proc_sigma[i] * es->proc_sigma[i];
        }
        fp.est_hist = d_ehist;
        fp.err_sq = d_esq;
        return FTMPC_OK;
    }
    int fetch(const Loop& q, const ftmpc_estimator* es) {
        if (!on) return FTMPC_OK;
        const size_t B = (size_t)q.B;
        LOOP_TRY(hist_get(q, es->est_hist, d_ehist, (size_t)q.T * B * 13));
        LOOP_TRY(hist_get(q, es->err_sq, d_esq, B * 4));
        LOOP_TRY(hist_get(q, es->xhat, d_xhat, B * 13));
        if (es->cov) LOOP_TRY(dev_get(q, h_cov.data(), d_cov.p, B * 78));
        return FTMPC_OK;
    }
    void unpack(const Loop& q, const ftmpc_estimator* es) {
        if (on && es->cov) ftmpc::unpack_kb(h_cov.data(), q.B, 78, es->cov);
    }
};

// Disturbance estimate (checked by the entry; it needs the estimator): P_xd [72][B] and P_dd [21][B] component-major, 0 and diag(p0^2)
// when none is handed over; the estimate itself [B][6] = (f^, t^), what the linearise kernel's DIST instantiations and
// ftmpc_diagnose_dist_kernel read; the gain slot [168][B] between the two passes of the update
struct DistStage {
    bool on = false;
    DevBuf<double> d_cross, d_covd, d_est, d_gain, d_fh, d_th;
    std::vector<double> h_cross, h_covd, h_est;
    ftmpc::DistParams dq{};

    // force / torque [B][3] each <-> the estimate [B][6]
    void est_copy(const Loop& q, const ftmpc_disturbance* db, bool in) {
        double* const part[2] = {db->force, db->torque};
        for (int64_t b = 0; b < q.B; ++b)
            for (int a = 0; a < 2; ++a)
                for (int k = 0; part[a] && k < 3; ++k) {
                    double& host = part[a][b * 3 + k];
                    double& slot = h_est[(size_t)b * 6 + 3 * a + k];
                    if (in) slot = host;
                    else host = slot;
                }
    }
    int stage(const Loop& q, const ftmpc_disturbance* db) {
        on = db != nullptr;
        if (!on) return FTMPC_OK;
        const int64_t B = q.B;
        try {
            h_cross.assign((size_t)B * 72, 0.0);
            h_covd.assign((size_t)B * 21, 0.0);
            h_est.assign((size_t)B * 6, 0.0);
        } catch (const std::bad_alloc&) {
            return fail(q.h, FTMPC_ERR_ALLOC, "out of host memory for the disturbance estimate's staging arrays");
        }
        if (db->cross) ftmpc::pack_kb(db->cross, B, 72, h_cross.data());
        if (db->cov) ftmpc::pack_kb(db->cov, B, 21, h_covd.data());
        if (!db->cov)
            for (int i = 0, k = 0; i < 6; k += 6 - i, ++i)
                std::fill(h_covd.begin() + (size_t)k * B, h_covd.begin() + (size_t)(k + 1) * B, db->p0[i / 3] * db->p0[i / 3]);
        est_copy(q, db, true);
        LOOP_TRY(dev_alloc(q, d_cross, (size_t)B * 72));
        LOOP_TRY(dev_alloc(q, d_covd, (size_t)B * 21));
        LOOP_TRY(dev_alloc(q, d_est, (size_t)B * 6));
        LOOP_TRY(dev_alloc(q, d_gain, (size_t)B * 168));
        LOOP_TRY(dev_put(q, d_cross.p, h_cross.data(), (size_t)B * 72));
        LOOP_TRY(dev_put(q, d_covd.p, h_covd.data(), (size_t)B * 21));
        LOOP_TRY(dev_put(q, d_est.p, h_est.data(), (size_t)B * 6));
        LOOP_TRY(hist_alloc(q, d_fh, db->force_hist, (size_t)q.T * B * 3));
        LOOP_TRY(hist_alloc(q, d_th, db->torque_hist, (size_t)q.T * B * 3));
        dq.cross = d_cross;
        dq.covd = d_covd;
        dq.dist = d_est;
        dq.gain = d_gain;
        for (int k = 0; k < 2; ++k) dq.qdsq[k] = db->proc_sigma[k] * db->proc_sigma[k];
        dq.force_hist = d_fh;
        dq.torque_hist = d_th;
        return FTMPC_OK;
    }
    int fetch(const Loop& q, const ftmpc_disturbance* db) {
        if (!on) return FTMPC_OK;
        const size_t B = (size_t)q.B;
        LOOP_TRY(hist_get(q, db->force_hist, d_fh, (size_t)q.T * B * 3));
        LOOP_TRY(hist_get(q, db->torque_hist, d_th, (size_t)q.T * B * 3));
        if (db->force || db->torque) LOOP_TRY(dev_get(q, h_est.data(), d_est.p, B * 6));
        if (db->cross) LOOP_TRY(dev_get(q, h_cross.data(), d_cross.p, B * 72));
        if (db->cov) LOOP_TRY(dev_get(q, h_covd.data(), d_covd.p, B * 21));
        return FTMPC_OK;
    }
    void unpack(const Loop& q, const ftmpc_disturbance* db) {
        if (!on) return;
        est_copy(q, db, false);
        if (db->cross) ftmpc::unpack_kb(h_cross.data(), q.B, 72, db->cross);
        if (db->cov) ftmpc::unpack_kb(h_covd.data(), q.B, 21, db->cov);
    }
};

// Bias estimate (checked by the entry; it needs the estimator and excludes the disturbance estimate): the pieces in measured
// coordinates, P_mb [72][B] and P_bb [21][B] component-major with P_mm in the filter's d_cov; b^ [B][6]; the gain slot [168][B].
// Without a handed cross the bias prior is independent of the state error, and the pieces are T diag(P_xx, P_bb) T'
struct BiasStage {
    bool on = false;
    DevBuf<double> d_cross, d_covb, d_est, d_gain, d_hist;
    std::vector<double> h_cross, h_covb;
    ftmpc::BiasParams bq{};

    int stage(const Loop& q, const ftmpc_bias_estimate* be) {
        on = be != nullptr;
        if (!on) return FTMPC_OK;
        const int64_t B = q.B;
        try {
            h_cross.assign((size_t)B * 72, 0.0);
            h_covb.assign((size_t)B * 21, 0.0);
        } catch (const std::bad_alloc&) {
            return fail(q.h, FTMPC_ERR_ALLOC, "out of host memory for the bias estimate's staging arrays");
        }
        const double pb[2] = {be->p0[0] * be->p0[0], be->p0[1] * be->p0[1]};
        if (be->cross) ftmpc::pack_kb(be->cross, B, 72, h_cross.data());
        if (be->cov) ftmpc::pack_kb(be->cov, B, 21, h_covb.data());
        if (!be->cov)
            for (int i = 0, k = 0; i < 6; k += 6 - i, ++i) std::fill(h_covb.begin() + (size_t)k * B, h_covb.begin() + (size_t)(k + 1) * B, pb[i / 3]);
        if (!be->cross) {
            for (int r = 0; r < 3; ++r) {
                const int kv = 6 * (3 + r) + r, kw = 6 * (9 + r) + 3 + r;      // HB's ones
                std::fill(h_cross.begin() + (size_t)kv * B, h_cross.begin() + (size_t)(kv + 1) * B, pb[0]);
                std::fill(h_cross.begin() + (size_t)kw * B, h_cross.begin() + (size_t)(kw + 1) * B, pb[1]);
            }
        }
        LOOP_TRY(dev_alloc(q, d_cross, (size_t)B * 72));
        LOOP_TRY(dev_alloc(q, d_covb, (size_t)B * 21));
        LOOP_TRY(dev_alloc(q, d_est, (size_t)B * 6));
        LOOP_TRY(dev_alloc(q, d_gain, (size_t)B * 168));
        LOOP_TRY(dev_put(q, d_cross.p, h_cross.data(), (size_t)B * 72));
        LOOP_TRY(dev_put(q, d_covb.p, h_covb.data(), (size_t)B * 21));
        if (be->bias)
            LOOP_TRY(dev_put(q, d_est.p, (const double*)be->bias, (size_t)B * 6));
        else
            LOOP_TRY(dev_fill(q, d_est.p, 0, (size_t)B * 6));
        LOOP_TRY(hist_alloc(q, d_hist, be->bias_hist, (size_t)q.T * B * 6));
        bq.cross = d_cross;
        bq.covb = d_covb;
        bq.bias = d_est;
        bq.gain = d_gain;
        for (int k = 0; k < 2; ++k) bq.qbsq[k] = be->proc_sigma[k] * be->proc_sigma[k];
        bq.bias_hist = d_hist;
        return FTMPC_OK;
    }
    int fetch(const Loop& q, const ftmpc_bias_estimate* be) {
        if (!on) return FTMPC_OK;
        const size_t B = (size_t)q.B;
        LOOP_TRY(hist_get(q, be->bias_hist, d_hist, (size_t)q.T * B * 6));
        LOOP_TRY(hist_get(q, be->bias, d_est, B * 6));
        if (be->cross) LOOP_TRY(dev_get(q, h_cross.data(), d_cross.p, B * 72));
        if (be->cov) LOOP_TRY(dev_get(q, h_covb.data(), d_covb.p, B * 21));
        return FTMPC_OK;
    }
    void unpack(const Loop& q, const ftmpc_bias_estimate* be) {
        if (!on) return;
        if (be->cross) ftmpc::unpack_kb(h_cross.data(), q.B, 72, be->cross);
        if (be->cov) ftmpc::unpack_kb(h_covb.data(), q.B, 21, be->cov);
    }
};

// Outage (checked by the entry; it needs the estimator and excludes both estimates): the chain's state [B][3], the counters [B][4]
// and the scripted window [B][2] in the caller's layout (a lane reads and writes its own few words once per step), zeros when none are
// handed over; the availability word [B] between ftmpc_outage_kernel and its two consumers; the four histories.  Nothing is converted
// on the way out, so there is no unpack
struct OutageStage {
    bool on = false;
    DevBuf<int32_t> d_avail, d_state, d_rej, d_out, d_win, d_ahist, d_ohist, d_ghist;
    DevBuf<double> d_mhist;
    ftmpc::OutageParams oq{};
    ftmpc::GateParams gq{};

    int stage(const Loop& q, const ftmpc_outage* og) {
        on = !outage_trivial(og);
        if (!on) return FTMPC_OK;
        const size_t T = (size_t)q.T, B = (size_t)q.B;
        auto counters = [&](DevBuf<int32_t>& d, const int32_t* host, size_t n) -> int {
            LOOP_TRY(dev_alloc(q, d, n));
            return host ? dev_put(q, d.p, host, n) : dev_fill(q, d.p, 0, n);
        };
        LOOP_TRY(dev_alloc(q, d_avail, B));
        LOOP_TRY(counters(d_state, og->state, B * 3));
        LOOP_TRY(counters(d_rej, og->rejected, B * 4));
        LOOP_TRY(counters(d_out, og->outliers, B * 4));
        if (og->window) {
            LOOP_TRY(dev_alloc(q, d_win, B * 2));
            LOOP_TRY(dev_put(q, d_win.p, og->window, B * 2));
        }
        LOOP_TRY(hist_alloc(q, d_ahist, (const int32_t*)og->avail_hist, T * B));
        LOOP_TRY(hist_alloc(q, d_ohist, (const int32_t*)og->outlier_hist, T * B));
        LOOP_TRY(hist_alloc(q, d_ghist, (const int32_t*)og->gate_hist, T * B));
        LOOP_TRY(hist_alloc(q, d_mhist, (const double*)og->meas_hist, T * B * 13));
        oq.B = q.B;
        oq.y = q.h->d_x0;
        oq.seed = og->seed;
        oq.p_loss = og->p_loss;
        oq.p_recover = og->p_recover;
        for (int k = 0; k < 4; ++k) {
            oq.p_outlier[k] = og->p_outlier[k];
            oq.outlier_sigma[k] = og->outlier_sigma[k];
        }
        oq.index0 = q.index0;
        oq.index_total = q.index_total;
        oq.window = d_win;
        oq.state = d_state;
        oq.outliers = d_out;
        oq.avail = d_avail;
        oq.avail_hist = d_ahist;
        oq.outlier_hist = d_ohist;
        oq.meas_hist = d_mhist;
        gq.avail = d_avail;
        gq.gate_sq = og->gate * og->gate;
        gq.rejected = d_rej;
        gq.gate_hist = d_ghist;
        return FTMPC_OK;
    }
    int fetch(const Loop& q, const ftmpc_outage* og) {
        if (!on) return FTMPC_OK;
        const size_t T = (size_t)q.T, B = (size_t)q.B;
        LOOP_TRY(hist_get(q, og->state, d_state, B * 3));
        LOOP_TRY(hist_get(q, og->rejected, d_rej, B * 4));
        LOOP_TRY(hist_get(q, og->outliers, d_out, B * 4));
        LOOP_TRY(hist_get(q, og->avail_hist, d_ahist, T * B));
        LOOP_TRY(hist_get(q, og->outlier_hist, d_ohist, T * B));
        LOOP_TRY(hist_get(q, og->gate_hist, d_ghist, T * B));
        LOOP_TRY(hist_get(q, og->meas_hist, d_mhist, T * B * 13));
        return FTMPC_OK;
    }
};

// Environment (checked by the entry): the wrench of the step, force [3][B] and torque [3][B], which simulate_core wires into the plant's
// PlantVar in place of PlantStage's constant arrays (those become the kernel's base); the Gauss-Markov state [6][B], the amplitudes
// [3][B] each and the kick [6][B] component-major, vehicle-major at the ABI; the phase [B], the window [B][2] and the error sums [B][2]
// in the caller's layout; phi and the innovation scale computed here, once per call
struct EnvironmentStage {
    bool on = false;
    DevBuf<double> d_force, d_torque, d_g, d_af, d_at, d_ph, d_kick, d_whist, d_err;
    DevBuf<int32_t> d_win;
    std::vector<double> h_g, h_af, h_at, h_kick;
    ftmpc::EnvParams eq{};

    int stage(const Loop& q, const ftmpc_environment* ev) {
        on = !environment_trivial(ev);
        if (!on) return FTMPC_OK;
        const size_t T = (size_t)q.T, B = (size_t)q.B;
        auto packed = [&](DevBuf<double>& d, const double* src, int64_t K, std::vector<double>& v) -> int {
            if (!src) return FTMPC_OK;
            v.resize(B * (size_t)K);
            ftmpc::pack_kb(src, q.B, K, v.data());
            LOOP_TRY(dev_alloc(q, d, v.size()));
            return dev_put(q, d.p, v.data(), v.size());
        };
        try {
            h_g.assign(B * 6, 0.0);      // (also the landing place of the state's read-back)
            LOOP_TRY(packed(d_af, ev->amp_force, 3, h_af));
            LOOP_TRY(packed(d_at, ev->amp_torque, 3, h_at));
            LOOP_TRY(packed(d_kick, ev->kick, 6, h_kick));
        } catch (const std::bad_alloc&) {
            return fail(q.h, FTMPC_ERR_ALLOC, "out of host memory for the environment's staging arrays");
        }
        LOOP_TRY(dev_alloc(q, d_force, B * 3));
        LOOP_TRY(dev_alloc(q, d_torque, B * 3));
        LOOP_TRY(dev_alloc(q, d_g, B * 6));
        if (ev->state) {
            ftmpc::pack_kb(ev->state, q.B, 6, h_g.data());
            LOOP_TRY(dev_put(q, d_g.p, h_g.data(), B * 6));
        }
        if (ev->phase) {
            LOOP_TRY(dev_alloc(q, d_ph, B));
            LOOP_TRY(dev_put(q, d_ph.p, ev->phase, B));
        }
        if (ev->window) {
            LOOP_TRY(dev_alloc(q, d_win, B * 2));
            LOOP_TRY(dev_put(q, d_win.p, ev->window, B * 2));
        }
        if (ev->est_err_sq) {
            LOOP_TRY(dev_alloc(q, d_err, B * 2));
            LOOP_TRY(dev_put(q, d_err.p, (const double*)ev->est_err_sq, B * 2));
        }
        LOOP_TRY(hist_alloc(q, d_whist, (const double*)ev->wrench_hist, T * B * 6));
        eq.B = q.B;
        eq.seed = ev->seed;
        eq.index0 = q.index0;
        eq.index_total = q.index_total;
        ftmpc_env::process(ev->sigma, ev->tau, q.h->cfg.dt, ev->period, eq.proc);
        eq.amp_f = d_af;
        eq.amp_t = d_at;
        eq.phase = d_ph;
        eq.kick = d_kick;
        eq.window = d_win;
        eq.g = d_g;
        eq.force = d_force;
        eq.torque = d_torque;
        eq.wrench_hist = d_whist;
        eq.err_sq = d_err;
        return FTMPC_OK;
    }
    int fetch(const Loop& q, const ftmpc_environment* ev) {
        if (!on) return FTMPC_OK;
        const size_t T = (size_t)q.T, B = (size_t)q.B;
        if (ev->state) LOOP_TRY(dev_get(q, h_g.data(), d_g.p, B * 6));
        LOOP_TRY(hist_get(q, ev->est_err_sq, d_err, B * 2));
        LOOP_TRY(hist_get(q, ev->wrench_hist, d_whist, T * B * 6));
        return FTMPC_OK;
    }
    void unpack(const Loop& q, const ftmpc_environment* ev) {
        if (on && ev->state) ftmpc::unpack_kb(h_g.data(), q.B, 6, ev->state);
    }
};

// Isolation (checked by the entry; it needs the diagnosis): the leader and its run [B][2], the void and the revision counts [B] in
// the caller's layout (a lane reads and writes its own few words once per step), (-1, 0) and zeros when none are handed over; the
// fit history.  Nothing is converted on the way out, so there is no unpack
struct IsolationStage {
    bool on = false;
    DevBuf<int32_t> d_lead, d_void, d_rev;
    DevBuf<double> d_fit;
    std::vector<int32_t> h_lead;
    ftmpc::IsoParams iq{};

    // force: a reinstating probe runs the rule's kernel whatever the struct says (NULL: the trivial rule)
    int stage(const Loop& q, const ftmpc_isolation* is, bool force) {
        on = !isolation_trivial(is) || force;
        if (!on) return FTMPC_OK;
        ftmpc_isolation none{};
        none.persist = 1;
        if (!is) is = &none;
        const size_t T = (size_t)q.T, B = (size_t)q.B;
        LOOP_TRY(dev_alloc(q, d_lead, B * 2));
        if (is->lead) {
            LOOP_TRY(dev_put(q, d_lead.p, (const int32_t*)is->lead, B * 2));
        } else {
            try {
                h_lead.assign(B * 2, 0);
            } catch (const std::bad_alloc&) {
                return fail(q.h, FTMPC_ERR_ALLOC, "out of host memory for the isolation's staging array");
            }
            for (size_t b = 0; b < B; ++b) h_lead[b * 2] = -1;
            LOOP_TRY(dev_put(q, d_lead.p, (const int32_t*)h_lead.data(), B * 2));
        }
        auto counters = [&](DevBuf<int32_t>& d, const int32_t* host) -> int {
            LOOP_TRY(dev_alloc(q, d, B));
            return host ? dev_put(q, d.p, host, B) : dev_fill(q, d.p, 0, B);
        };
        LOOP_TRY(counters(d_void, is->voided));
        LOOP_TRY(counters(d_rev, is->revised));
        LOOP_TRY(hist_alloc(q, d_fit, (const double*)is->fit_hist, T * B * 2));
        iq.consist_sq = is->consist * is->consist;
        iq.persist = is->persist;
        iq.revise = is->revise;
        iq.lead = d_lead;
        iq.voided = d_void;
        iq.revised = d_rev;
        iq.fit_hist = d_fit;
        return FTMPC_OK;
    }
    int fetch(const Loop& q, const ftmpc_isolation* is) {
        if (!on || !is) return FTMPC_OK;
        const size_t T = (size_t)q.T, B = (size_t)q.B;
        LOOP_TRY(hist_get(q, is->lead, d_lead, B * 2));
        LOOP_TRY(hist_get(q, is->voided, d_void, B));
        LOOP_TRY(hist_get(q, is->revised, d_rev, B));
        LOOP_TRY(hist_get(q, is->fit_hist, d_fit, T * B * 2));
        return FTMPC_OK;
    }
};

// Probe (checked by the entry; it needs the diagnosis): the counters idle and pulses [B][NT] and reinstated [B] in the caller's layout,
// impulse [B], pacc and health component-major [NT][B] as the diagnosis' acc and llr are (zeros when none are handed over), the
// pulsed thruster of every step [T][B].  The pointers into the diagnosis' pattern and detection list are set by the wiring
struct ProbeStage {
    bool on = false;
    DevBuf<int32_t> d_idle, d_pulses, d_rein, d_hist;
    DevBuf<double> d_impulse, d_pacc, d_health;
    std::vector<double> h_pacc, h_health;
    ftmpc::ProbeParams pq{};

    int stage(const Loop& q, const ftmpc_probe* pb, const ftmpc_diagnosis* dg) {
        on = pb != nullptr;
        if (!on) return FTMPC_OK;
        const size_t T = (size_t)q.T, B = (size_t)q.B, NT = (size_t)q.NT;
        try {
            if (pb->pacc) h_pacc.assign(B * NT, 0.0);
            if (pb->health) h_health.assign(B * NT, 0.0);
        } catch (const std::bad_alloc&) {
            return fail(q.h, FTMPC_ERR_ALLOC, "out of host memory for the probe's staging arrays");
        }
        auto counters = [&](DevBuf<int32_t>& d, const int32_t* host, size_t n) -> int {
            LOOP_TRY(dev_alloc(q, d, n));
            return host ? dev_put(q, d.p, host, n) : dev_fill(q, d.p, 0, n);
        };
        auto sums = [&](DevBuf<double>& d, const double* host, std::vector<double>& packed) -> int {
            LOOP_TRY(dev_alloc(q, d, B * NT));
            if (!host) return dev_fill(q, d.p, 0, B * NT);
            ftmpc::pack_kb(host, q.B, q.NT, packed.data());
            return dev_put(q, d.p, (const double*)packed.data(), B * NT);
        };
        LOOP_TRY(counters(d_idle, pb->idle, B * NT));
        LOOP_TRY(counters(d_pulses, pb->pulses, B * NT));
        LOOP_TRY(counters(d_rein, pb->reinstated, B));
        LOOP_TRY(dev_alloc(q, d_impulse, B));
        if (pb->impulse)
            LOOP_TRY(dev_put(q, d_impulse.p, (const double*)pb->impulse, B));
        else
            LOOP_TRY(dev_fill(q, d_impulse.p, 0, B));
        LOOP_TRY(sums(d_pacc, pb->pacc, h_pacc));
        LOOP_TRY(sums(d_health, pb->health, h_health));
        LOOP_TRY(hist_alloc(q, d_hist, (const int32_t*)pb->thruster_hist, T * B));
        pq.B = q.B;
        pq.amp = pb->amp, pq.quiet = pb->quiet, pq.restore_ub = pb->reinstate ? pb->restore_ub : 0.0, pq.dt = q.h->cfg.dt;
        pq.idle_steps = pb->idle_steps, pq.max_pulses = pb->max_pulses, pq.reinstate = pb->reinstate, pq.n_levels = dg->n_levels;
        pq.K = dg->max_detect;
        pq.u0 = q.h->d_u0;
        pq.ub = q.h->d_ub;
        pq.idle = d_idle;
        pq.pulses = d_pulses;
        pq.impulse = d_impulse;
        pq.pacc = d_pacc;
        pq.health = d_health;
        pq.reinstated = d_rein;
        pq.hist = d_hist;
        return FTMPC_OK;
    }
    int fetch(const Loop& q, const ftmpc_probe* pb) {
        if (!on) return FTMPC_OK;
        const size_t T = (size_t)q.T, B = (size_t)q.B, NT = (size_t)q.NT;
        LOOP_TRY(hist_get(q, pb->idle, d_idle, B * NT));
        LOOP_TRY(hist_get(q, pb->pulses, d_pulses, B * NT));
        LOOP_TRY(hist_get(q, pb->reinstated, d_rein, B));
        LOOP_TRY(hist_get(q, pb->impulse, d_impulse, B));
        if (pb->pacc) LOOP_TRY(dev_get(q, h_pacc.data(), (const double*)d_pacc.p, B * NT));
        if (pb->health) LOOP_TRY(dev_get(q, h_health.data(), (const double*)d_health.p, B * NT));
        LOOP_TRY(hist_get(q, pb->thruster_hist, d_hist, T * B));
        return FTMPC_OK;
    }
    void unpack(const Loop& q, const ftmpc_probe* pb) {
        if (!on) return;
        if (pb->pacc) ftmpc::unpack_kb(h_pacc.data(), q.B, q.NT, pb->pacc);
        if (pb->health) ftmpc::unpack_kb(h_health.data(), q.B, q.NT, pb->health);
    }
};

// Diagnosis (checked by the entry): xt and n [B][14], acc [NT][B] and the statistics [H][B] component-major (filled on the device when
// none are handed over), the detect arrays [B][K] with the count per vehicle, the flag the repair kernel reads.  On the wrench form
// also the hull rebuild: the new offsets [B][hull_rows] and [flat B | no_hull B]
struct DiagStage {
    bool on = false;
    int L = 0, K = 0;      // levels, detections kept per vehicle
    int64_t H = 0;         // statistics per vehicle
    DevBuf<double> d_xt, d_acc, d_llr, d_hist, d_hbnew;
    DevBuf<int32_t> d_det;      // [count B | switched B | step BK | thruster BK | level BK]
    DevBuf<int32_t> d_hflat;
    std::vector<double> h_state, h_xt, h_acc, h_llr;
    std::vector<int32_t> h_det;
    ftmpc::DiagParams dp{};
    ftmpc::HullOffsets ho{};
    ftmpc::HullSwitch hw{};

    int stage(const Loop& q, const ftmpc_diagnosis* dg, const LoopCall& c) {
        on = dg != nullptr;
        if (!on) return FTMPC_OK;
        const int64_t B = q.B;
        const int NT = q.NT;
        L = dg->n_levels, K = dg->max_detect, H = (int64_t)NT * L;
        const size_t nd = (size_t)B * (2 + 3 * (size_t)K);
        const bool llr_in = dg->state && dg->llr;
        try {
            h_xt.assign((size_t)B * 14, 0.0);
            h_acc.assign((size_t)B * NT, 0.0);
            if (llr_in) h_llr.assign((size_t)(B * H), 0.0);
            h_det.assign(nd, -1);
        } catch (const std::bad_alloc&) {
            return fail(q.h, FTMPC_ERR_ALLOC, "out of host memory for the diagnosis' staging arrays");
        }
        std::fill(h_det.begin(), h_det.begin() + 2 * B, 0);
        LOOP_TRY(dev_alloc(q, d_xt, (size_t)B * 14));
        LOOP_TRY(dev_alloc(q, d_acc, (size_t)B * NT));
        LOOP_TRY(dev_alloc(q, d_llr, (size_t)(B * H)));
        LOOP_TRY(dev_alloc(q, d_det, nd));
        if (dg->state) {
            const int64_t w = 14 + NT;
            for (int64_t b = 0; b < B; ++b) {
                for (int k = 0; k < 14; ++k) h_xt[(size_t)b * 14 + k] = dg->state[b * w + k];
                for (int i = 0; i < NT; ++i) h_acc[(size_t)i * B + b] = dg->state[b * w + 14 + i];
                int32_t cnt = 0;
                for (int k = 0; k < K; ++k) {
                    const int32_t ds = dg->detect_step[b * K + k];
                    h_det[(size_t)(2 * B + b * K + k)] = ds;
                    h_det[(size_t)(2 * B + (B + b) * K + k)] = ds < 0 ? -1 : dg->detect_thruster[b * K + k];
                    h_det[(size_t)(2 * B + (2 * B + b) * K + k)] = ds < 0 ? -1 : dg->detect_level[b * K + k];
                    cnt += ds >= 0;
                }
                h_det[(size_t)b] = cnt;
            }
            LOOP_TRY(dev_put(q, d_xt.p, h_xt.data(), h_xt.size()));
            LOOP_TRY(dev_put(q, d_acc.p, h_acc.data(), h_acc.size()));
        } else {      // (the first step's phase 0 initialises both)
            LOOP_TRY(dev_fill(q, d_xt.p, 0, (size_t)B * 14));
            LOOP_TRY(dev_fill(q, d_acc.p, 0, (size_t)B * NT));
        }
        if (llr_in) {
            ftmpc::pack_kb(dg->llr, B, H, h_llr.data());
            LOOP_TRY(dev_put(q, d_llr.p, h_llr.data(), h_llr.size()));
        } else {
            LOOP_TRY(dev_fill(q, d_llr.p, 0, (size_t)(B * H)));
        }
        LOOP_TRY(dev_put(q, d_det.p, h_det.data(), nd));
        LOOP_TRY(hist_alloc(q, d_hist, dg->llr_hist, (size_t)(q.T * B * H)));
        dp.B = B;
        dp.L = L;
        dp.K = K;
        dp.xt = d_xt;
        dp.acc = d_acc;
        dp.llr = d_llr;
        for (int l = 0; l < L; ++l) dp.levels[l] = dg->levels[l];
        for (int k = 0; k < 2; ++k) {
            dp.rsq[k] = dg->resid_sigma[k] * dg->resid_sigma[k];
            dp.dsq[k] = dg->drift_sigma[k] * dg->drift_sigma[k];
        }
        dp.threshold = dg->threshold;
        dp.ub = q.h->d_ub;
        dp.stuck = q.h->d_stuck;
        dp.count = d_det;
        dp.switched = d_det + B;
        dp.det_step = d_det + 2 * B;
        dp.det_thruster = d_det + 2 * B + B * K;
        dp.det_level = d_det + 2 * B + 2 * B * K;
        dp.llr_hist = d_hist;
        return c.wrench ? stage_hull(q, c) : FTMPC_OK;
    }
    int stage_hull(const Loop& q, const LoopCall& c) {
        const int64_t B = q.B;
        const int R = c.hull_rows;
        ftmpc_handle* h = q.h;
        LOOP_TRY(dev_alloc(q, d_hbnew, (size_t)B * R));
        LOOP_TRY(dev_alloc(q, d_hflat, 2 * (size_t)B));
        if (c.no_hull_step)
            LOOP_TRY(dev_put(q, d_hflat + B, (const int32_t*)c.no_hull_step, (size_t)B));
        else
            LOOP_TRY(dev_fill(q, d_hflat + B, 0xFF, (size_t)B));
        ho.B = B;
        ho.hull_rows = R;
        ho.switched = dp.switched;
        ho.ub = h->d_ub;
        ho.stuck = h->d_stuck;
        ho.hullA = h->d_hullA;
        ho.hullset = c.hull_set ? h->d_hullset.p : nullptr;
        ho.out_b = d_hbnew;
        ho.flat = d_hflat;
        hw.B = B;
        hw.hull_rows = R;
        hw.switched = dp.switched;
        hw.flat = d_hflat;
        hw.ub = h->d_ub;
        hw.stuck = h->d_stuck;
        hw.hullA = h->d_hullA;
        hw.hullset = ho.hullset;
        hw.new_b = d_hbnew;
        hw.hullb = h->d_hullb;
        hw.warmG = h->d_warmG;
        hw.no_hull = d_hflat + B;
        return FTMPC_OK;
    }
    int fetch(const Loop& q, const ftmpc_diagnosis* dg, const LoopCall& c) {
        if (!on) return FTMPC_OK;
        const size_t B = (size_t)q.B;
        LOOP_TRY(hist_get(q, dg->llr_hist, d_hist, (size_t)(q.T * q.B * H)));
        if (dg->ub) LOOP_TRY(dev_get(q, dg->ub, q.h->d_ub.p, B * q.NT));
        if (dg->stuck) LOOP_TRY(dev_get(q, dg->stuck, q.h->d_stuck.p, B * q.NT));
        if (dg->state) {
            LOOP_TRY(dev_get(q, h_xt.data(), d_xt.p, h_xt.size()));
            LOOP_TRY(dev_get(q, h_acc.data(), d_acc.p, h_acc.size()));
            LOOP_TRY(dev_get(q, h_det.data(), d_det.p, h_det.size()));
            if (dg->llr) LOOP_TRY(dev_get(q, h_llr.data(), d_llr.p, h_llr.size()));
        }
        if (c.wrench && c.no_hull_step) LOOP_TRY(dev_get(q, c.no_hull_step, d_hflat + B, B));
        return FTMPC_OK;
    }
    void unpack(const Loop& q, const ftmpc_diagnosis* dg) {
        if (!on || !dg->state) return;
        const int64_t B = q.B, w = 14 + q.NT;
        for (int64_t b = 0; b < B; ++b) {
            for (int k = 0; k < 14; ++k) dg->state[b * w + k] = h_xt[(size_t)b * 14 + k];
            for (int i = 0; i < q.NT; ++i) dg->state[b * w + 14 + i] = h_acc[(size_t)i * B + b];
            for (int k = 0; k < K; ++k) {
                dg->detect_step[b * K + k] = h_det[(size_t)(2 * B + b * K + k)];
                dg->detect_thruster[b * K + k] = h_det[(size_t)(2 * B + (B + b) * K + k)];
                dg->detect_level[b * K + k] = h_det[(size_t)(2 * B + (2 * B + b) * K + k)];
            }
        }
        if (dg->llr) ftmpc::unpack_kb(h_llr.data(), B, H, dg->llr);
    }
};

// Mission (checked by the entry): reference tables with a table number and a start column per vehicle, gathered into per-vehicle
// windows before every solve (ftmpc::RefWindow), and / or the closed-loop cost.  Without tables and without cost nothing differs
// from a call without the struct
struct MissionStage {
    DevBuf<double> d_tab, d_utab, d_xwin, d_uwin, d_qprev, d_cost;
    DevBuf<int32_t> d_tbl, d_off;
    ftmpc::RefWindow rw{};
    ftmpc::MissionOut mo{};

    // xw, uw: doubles per window; L: the columns a predicting sensor shifts every window by
    int stage(const Loop& q, const ftmpc_mission* ms, bool windows, bool want_cost, int64_t xw, int64_t uw, int L) {
        const size_t B = (size_t)q.B;
        if (windows) {
            const size_t KC = (size_t)ms->n_tables * (size_t)ms->n_cols;
            LOOP_TRY(dev_alloc(q, d_tab, KC * 9));
            LOOP_TRY(dev_put(q, d_tab.p, ms->xref, KC * 9));
            LOOP_TRY(dev_alloc(q, d_xwin, (size_t)(q.B * xw)));
            if (ms->uref) {
                LOOP_TRY(dev_alloc(q, d_utab, KC * 6));
                LOOP_TRY(dev_put(q, d_utab.p, ms->uref, KC * 6));
                LOOP_TRY(dev_alloc(q, d_uwin, (size_t)(q.B * uw)));
            }
            if (ms->table) {
                LOOP_TRY(dev_alloc(q, d_tbl, B));
                LOOP_TRY(dev_put(q, d_tbl.p, ms->table, B));
            }
            if (ms->offset) {
                LOOP_TRY(dev_alloc(q, d_off, B));
                LOOP_TRY(dev_put(q, d_off.p, ms->offset, B));
            }
            rw.B = q.B;
            rw.C = ms->n_cols;
            rw.N1 = q.N + 1 + L;
            rw.xtab = d_tab;
            rw.utab = d_utab;
            rw.table = d_tbl;
            rw.offset = d_off;
            rw.xwin = d_xwin;
            rw.uwin = d_uwin;
        }
        if (want_cost) {     // the three sums, and q_0 of every vehicle from the staged x (pitch 13 -> 4 doubles)
            LOOP_TRY(dev_alloc(q, d_cost, B * 3));
            LOOP_TRY(dev_fill(q, d_cost.p, 0, B * 3));
            LOOP_TRY(dev_alloc(q, d_qprev, B * 4));
            HIP_TRY(q.h, hipMemcpy2DAsync(d_qprev, 4 * sizeof(double), q.h->d_x0 + 6, 13 * sizeof(double), 4 * sizeof(double), B,
                                          hipMemcpyDeviceToDevice, q.s));
            mo.cost = d_cost;
            mo.qprev = d_qprev;
            mo.tcost = q.h->d_tcost;
        }
        return FTMPC_OK;
    }
    int fetch(const Loop& q, const ftmpc_mission* ms, bool want_cost) { return want_cost ? dev_get(q, ms->cost, d_cost.p, (size_t)q.B * 3) : FTMPC_OK; }
};

// Outcomes: records [err_int 3 | err_max 3 | impulse 2] x B and [settle | tset | unsolved | first_unsolved | alloc_failed] x B, the
// terminal rows of the config, the status history.  on: some record is asked for, or the mission's cost (which the outcome kernel sums)
struct OutcomeStage {
    bool on = false;
    DevBuf<double> d_rec, d_term;
    DevBuf<int32_t> d_int, d_shist;
    ftmpc::OutcomeParams op{};

    int stage(const Loop& q, const ftmpc_outcomes* oc, bool want_cost, bool wrench) {
        const bool want_rec = oc && (oc->err_int || oc->err_max || oc->impulse || oc->settle_step || oc->tset_step || oc->unsolved ||
                                     oc->first_unsolved || oc->alloc_failed);
        on = want_rec || (oc && oc->status_hist) || want_cost;
        if (!on) return FTMPC_OK;
        const int64_t B = q.B;
        ftmpc_handle* h = q.h;
        LOOP_TRY(dev_alloc(q, d_rec, (size_t)B * 8));
        LOOP_TRY(dev_alloc(q, d_int, (size_t)B * 5));
        LOOP_TRY(dev_fill(q, d_rec.p, 0, (size_t)B * 8));
        LOOP_TRY(dev_fill(q, d_int.p, 0, (size_t)B * 5));
        LOOP_TRY(dev_fill(q, d_int + B, 0xFF, (size_t)B));          // tset_step = -1
        LOOP_TRY(dev_fill(q, d_int + 3 * B, 0xFF, (size_t)B));      // first_unsolved = -1
        op.B = B;
        op.u0 = h->d_u0;
        op.astatus = wrench ? h->d_ast2.p : nullptr;
        op.err_int = d_rec;
        op.err_max = d_rec + 3 * B;
        op.impulse = d_rec + 6 * B;
        op.settle = d_int;
        op.tset = d_int + B;
        op.unsolved = d_int + 2 * B;
        op.first_unsolved = d_int + 3 * B;
        op.alloc_failed = d_int + 4 * B;
        if (oc && oc->settle_step) {
            op.tol[0] = oc->tol_pos;
            op.tol[1] = oc->tol_vel;
            op.tol[2] = oc->tol_rate;
        }
        if (oc && oc->tset_step) {
            const int R = h->cfg.term_rows;
            LOOP_TRY(dev_alloc(q, d_term, (size_t)R * 10));
            LOOP_TRY(dev_put(q, d_term.p, (const double*)h->cfg.term_A, (size_t)R * 9));
            LOOP_TRY(dev_put(q, d_term + R * 9, (const double*)h->cfg.term_b, (size_t)R));
            op.term = d_term;
            op.term_rows = R;
        }
        if (oc && oc->status_hist) {
            LOOP_TRY(dev_alloc(q, d_shist, (size_t)q.T * B));
            op.status_hist = d_shist;
        }
        return FTMPC_OK;
    }
    int fetch(const Loop& q, const ftmpc_outcomes* oc) {
        if (!on || !oc) return FTMPC_OK;
        const int64_t B = q.B;
        double* const rec[3] = {oc->err_int, oc->err_max, oc->impulse};
        const int64_t rec_off[3] = {0, 3 * B, 6 * B}, rec_n[3] = {3 * B, 3 * B, 2 * B};
        for (int i = 0; i < 3; ++i)
            if (rec[i]) LOOP_TRY(dev_get(q, rec[i], d_rec + rec_off[i], (size_t)rec_n[i]));
        int32_t* const cnt[5] = {oc->settle_step, oc->tset_step, oc->unsolved, oc->first_unsolved, oc->alloc_failed};
        for (int i = 0; i < 5; ++i)
            if (cnt[i]) LOOP_TRY(dev_get(q, cnt[i], d_int + i * B, (size_t)B));
        return hist_get(q, oc->status_hist, d_shist, (size_t)q.T * B);
    }
};

// Fault schedule (E > 0): events [on | de | hull_set], patterns [ub | stuck], hull offsets; and the plant's own pattern [ub | stuck],
// which a schedule or a diagnosis splits from the controller's (own_pattern)
struct FaultStage {
    int E = 0;
    bool own_pattern = false;
    DevBuf<int32_t> d_ev;
    DevBuf<double> d_pat, d_hb, d_plant;
    std::vector<char> ev_step;         // steps at which some instance switches its plant or controller pattern
    std::vector<int32_t> ev;           // the staged events: an asynchronous copy reads them
    ftmpc::FaultEvents fe{};

    int stage(const Loop& q, const ftmpc_fault_schedule* fs, const LoopCall& c, bool diag) {
        E = fs ? fs->n_events : 0;
        own_pattern = E > 0 || diag;
        if (!own_pattern) return FTMPC_OK;
        const int64_t B = q.B;
        const int NT = q.NT;
        ftmpc_handle* h = q.h;
        LOOP_TRY(dev_alloc(q, d_plant, (size_t)B * NT * 2));
        LOOP_TRY(dev_put(q, d_plant.p, c.ub, (size_t)B * NT));
        LOOP_TRY(dev_put(q, d_plant + B * NT, c.stuck, (size_t)B * NT));
        if (E == 0) return FTMPC_OK;      // (a diagnosis alone: the plant keeps the call's pattern whatever it makes of the controller's)
        const int64_t BE = B * E;
        ev.assign((size_t)BE * 3, 0);
        ev_step.assign((size_t)q.T, 0);
        for (int64_t i = 0; i < BE; ++i) {
            ev[i] = fs->onset[i];
            // (under a diagnosis the schedule moves the plant only: no event is ever detected, and only onset steps launch the kernel)
            ev[BE + i] = diag ? INT32_MAX : (fs->detect ? fs->detect[i] : fs->onset[i]);
            if (c.wrench && fs->hull_set) ev[2 * BE + i] = fs->hull_set[i];
            if (ev[i] >= 0 && ev[i] < q.T) ev_step[ev[i]] = 1;
            if (ev[i] >= 0 && ev[BE + i] < q.T) ev_step[ev[BE + i]] = 1;
        }
        LOOP_TRY(dev_alloc(q, d_ev, ev.size()));
        LOOP_TRY(dev_alloc(q, d_pat, (size_t)BE * NT * 2));
        LOOP_TRY(dev_put(q, d_ev.p, (const int32_t*)ev.data(), ev.size()));
        LOOP_TRY(dev_put(q, d_pat.p, fs->ub, (size_t)BE * NT));
        LOOP_TRY(dev_put(q, d_pat + BE * NT, fs->stuck, (size_t)BE * NT));
        if (c.wrench && !diag) {     // (under a diagnosis no event is detected: the schedule carries no hull tables)
            LOOP_TRY(dev_alloc(q, d_hb, (size_t)BE * c.hull_rows));
            LOOP_TRY(dev_put(q, d_hb.p, fs->hull_b, (size_t)BE * c.hull_rows));
        }
        fe.B = B;
        fe.E = E;
        fe.onset = d_ev;
        fe.detect = d_ev + BE;
        fe.ev_ub = d_pat;
        fe.ev_stuck = d_pat + BE * NT;
        fe.plant_ub = d_plant;
        fe.plant_stuck = d_plant + B * NT;
        fe.ub = h->d_ub;
        fe.stuck = h->d_stuck;
        if (c.wrench) {
            fe.warmG = h->d_warmG;
            fe.hullA = h->d_hullA;
            fe.ev_hullset = fs->hull_set ? d_ev + 2 * BE : nullptr;
            fe.ev_hullb = d_hb;
            fe.hullset = c.hull_set ? h->d_hullset.p : nullptr;
            fe.hullb = h->d_hullb;
            fe.hull_rows = c.hull_rows;
        }
        return FTMPC_OK;
    }
};

// The closed loop itself: everything is staged on h->stream, the T steps are enqueued, the results are read back, one synchronise.
// The caller has checked the arguments and made room on the handle (ftmpc_reserve or wrench_prepare).
int simulate_core(ftmpc_handle* h, const LoopCall& c) {
    int rc;
    const int N = h->cfg.N, NT = h->cfg.NT;
    const int64_t B = c.B;
    const int32_t T = c.T, sqp_iters = c.sqp_iters, backtracks = c.backtracks;
    const bool wrench = c.wrench, has_set = c.hull_set != nullptr;
    const ftmpc_estimator* const es = c.es;
    const ftmpc_diagnosis* const dg = c.dg;
    const ftmpc_disturbance* const db = c.db;
    const ftmpc_sensor* se = c.se;
    hipStream_t s = h->stream;
    // estimator: ftmpc_filter_kernel runs between the sense kernel and the solve (phase 0) and after the plant step (phase 1).  It
    // takes the truth-buffer path of a sensor even when the sensor is trivial or NULL (se0: latency 0, step0 0, nothing drawn); the
    // sense kernel then does not run and y_t is the truth
    const bool est = es != nullptr, dist = db != nullptr, bias = c.be != nullptr;
    // diagnosis: ftmpc_diagnose_kernel runs before the filter's phase 0 (phase 0) and after the plant step (phase 1); it takes the same
    // truth-buffer path.  On the wrench form ftmpc_hull_offsets_kernel and ftmpc_hull_switch_kernel follow phase 0: the offsets of the
    // vehicles that switched, from the pattern the controller now holds
    const bool diag = dg != nullptr;
    const bool sensing = !sensor_trivial(se);      // ftmpc_sense_kernel runs
    ftmpc_sensor se0{};
    if ((est || diag) && !se) se = &se0;
    const bool sense = sensing || est || diag;
    // a predicting sensor shifts every reference window by L = lat columns
    const int lat = sense ? se->latency : 0, L = sense && se->predict ? lat : 0;
    const int64_t ncol = (int64_t)T + N + L;   // windows t .. t+N for t < T (t+L .. t+L+N under a predicting sensor)
    const int64_t xw = 9 * (int64_t)(N + 1 + L), uw = 6 * (int64_t)(N + 1 + L);     // doubles per window
    const bool windows = c.ms && c.ms->n_tables > 0, want_cost = c.ms && c.ms->cost;
    const bool has_uref = windows ? c.ms->uref != nullptr : c.uref_traj != nullptr;
    const size_t nu = (size_t)B * NT;       // doubles per ring slot
    const Loop q{h, s, B, T, N, NT, c.oc ? c.oc->index0 : 0, c.oc && c.oc->index_total != 0 ? c.oc->index_total : B};

    // ---- staging (run before sen and mis: it puts x into h->d_x0, which the sensor and the mission's cost copy on the device)
    PlantStage pla;
    RunStage run;
    ActuatorStage act;
    SensorStage sen;
    FilterStage fil;
    DistStage dst;
    BiasStage bia;
    OutageStage oge;
    EnvironmentStage env;
    IsolationStage iso;
    ProbeStage prb;
    DiagStage dia;
    MissionStage mis;
    OutcomeStage out;
    FaultStage flt;
    LOOP_TRY(pla.stage(q, c.pm));
    LOOP_TRY(run.stage(q, c, windows, ncol));
    LOOP_TRY(act.stage(q, c.ac));
    LOOP_TRY(sen.stage(q, se, sense));
    LOOP_TRY(fil.stage(q, es, c.be, se));
    LOOP_TRY(dst.stage(q, db));
    LOOP_TRY(bia.stage(q, c.be));
    LOOP_TRY(oge.stage(q, c.og));
    LOOP_TRY(env.stage(q, c.ev));
    const bool reinstating = c.pb && c.pb->reinstate == 1;      // ftmpc_diagnose_probe_kernel is the call's phase-0 diagnosis kernel
    LOOP_TRY(iso.stage(q, c.is, reinstating));
    LOOP_TRY(prb.stage(q, c.pb, dg));
    LOOP_TRY(dia.stage(q, dg, c));
    LOOP_TRY(mis.stage(q, c.ms, windows, want_cost, xw, uw, L));
    LOOP_TRY(out.stage(q, c.oc, want_cost, wrench));
    LOOP_TRY(flt.stage(q, c.fs, c, diag));
    ftmpc::SenseParams& sn = sen.sn;
    ftmpc::FilterParams& fp = fil.fp;
    ftmpc::DiagParams& dp = dia.dp;
    ftmpc::HullSwitch& hw = dia.hw;
    ftmpc::RefWindow& rw = mis.rw;
    ftmpc::MissionOut& mo = mis.mo;
    ftmpc::OutcomeParams& op = out.op;
    ftmpc::FaultEvents& fe = flt.fe;
    double* const d_warmB = run.d_warmB.p;
    double* const d_ring = sen.d_ring.p;
    double* const d_dest = dst.d_est.p;

    // a continued run (step0 > 0, and the handle's last loop with a sensor ended at that step, on this batch and form, in this x):
    // its first solve is warm-started as the whole run's would be, from what the handle kept; otherwise it starts cold
    const int64_t nkeep = B * (int64_t)N * (wrench ? 6 : NT);
    bool resume = false;
    if (sense) {
        resume = se->step0 > 0 && h->keep_step == se->step0 && h->keep_B == B && h->keep_wrench == wrench &&
                 h->keep_x.size() == (size_t)B * 13 && std::memcmp(h->keep_x.data(), c.x, (size_t)B * 13 * sizeof(double)) == 0;
        h->keep_step = -1;      // valid again only when this call ends well
        if (resume)
            HIP_TRY(h, hipMemcpyAsync(wrench ? h->d_warmG.p : d_warmB, h->d_keep_warm, (size_t)nkeep * sizeof(double), hipMemcpyDeviceToDevice, s));
    }

    // ---- the wiring between the features' parameter blocks
    double* const d_truth = sense ? sen.d_xtrue.p : h->d_x0.p;      // what the plant integrates and the outcomes measure
    if (est) {
        sn.predict = 0;             // the filter propagates its own estimate over the queue, and writes pred_hist
        sn.pred_hist = nullptr;
        fp.y = sensing ? h->d_x0.p : sen.d_xtrue.p;
        fp.truth = sen.d_xtrue;
        fp.ring = sen.d_ring;
        fp.pred_hist = sen.d_phist;
    }
    if (diag) dp.y = sensing ? h->d_x0.p : sen.d_xtrue.p;
    if (oge.on) {     // ftmpc_outage_kernel rewrites y_t into the handle's x0 (from there, or from the truth): both consumers read it there
        oge.oq.src = fp.y;
        fp.y = h->d_x0;
        if (diag) dp.y = h->d_x0;
    }
    if (env.on) {     // ftmpc_environment_kernel writes the step's wrench where the plant reads its disturbance; the call's constant is its base
        env.eq.base_f = pla.pv.force;
        env.eq.base_t = pla.pv.torque;
        pla.pv.force = env.d_force;
        pla.pv.torque = env.d_torque;
        pla.var = true;
        env.eq.est = dist ? d_dest : nullptr;
    }
    if (prb.on) {     // the probe reads the controller's pattern and the diagnosis' detection list
        prb.pq.count = dp.count;
        prb.pq.det_thruster = dp.det_thruster;
        prb.pq.det_level = dp.det_level;
    }
    if (flt.E > 0) fe.warmU = wrench ? nullptr : d_warmB;
    ftmpc::SimParams sp;
    sp.B = B;
    sp.x = d_truth;
    sp.u0 = h->d_u0;
    sp.ub = h->d_ub;
    sp.stuck = h->d_stuck;
    if (flt.own_pattern) {     // the plant keeps its own pattern, whatever the schedule's detections or the diagnosis make of the controller's
        sp.ub = flt.d_plant;
        sp.stuck = flt.d_plant + B * NT;
    }
    for (int i = 0; i < 4; ++i) sp.noise[i] = c.noise[i];
    sp.seed = c.seed;
    sp.u_hist = run.d_hist;
    sp.status = h->d_status;
    sp.bad_count = run.d_bad;
    sp.index0 = q.index0;
    sp.index_total = q.index_total;
    sp.x_hist = run.d_xhist;
    if (out.on) op.x = d_truth;

    // ---- the steps
    const dim3 wave(64), per_vehicle((unsigned)((B + 63) / 64)), per_stage((unsigned)((B * N + 63) / 64));
    for (int t = 0; t < T; ++t) {
        if (flt.E > 0 && flt.ev_step[t]) {     // some instance switches its pattern at this step: before the solve
            fe.t = t;
            fe.repair = t > 0 || resume;
            hipLaunchKernelGGL(ftmpc::ftmpc_fault_event_kernel, per_stage, wave, 0, s, h->dc, fe);
            HIP_TRY(h, hipGetLastError());
            // the work lists follow the new patterns: no small grid for a list that was empty the step before
            h->qcnt_valid = false;
            h->qcnt_pending = false;
        }
        // window t..t+N of the reference (column-major, so a plain pointer offset; under a mission with tables: every vehicle's own
        // window, gathered here); warm start from step 1 on
        if (windows) {
            rw.t = t;
            const int64_t nwin = B * (xw + (rw.utab ? uw : 0));
            hipLaunchKernelGGL(ftmpc::ftmpc_ref_window_kernel, dim3((unsigned)((nwin + 255) / 256)), dim3(256), 0, s, rw);
            HIP_TRY(h, hipGetLastError());
        }
        // (under a predicting sensor the solve's window starts L columns later; xo_t / uo_t: the step's own columns, for the outcomes)
        const double* const xo_t = windows ? mis.d_xwin.p : run.d_xr + (int64_t)9 * t;
        const double* const uo_t = !has_uref ? nullptr : (windows ? mis.d_uwin.p : run.d_ur + (int64_t)6 * t);
        const double* const xr_t = xo_t + (int64_t)9 * L;
        const double* const ur_t = uo_t ? uo_t + (int64_t)6 * L : nullptr;
        if (sensing) {     // y_t (and its propagation over the queue) into h->d_x0; slot t mod (lat + 1) holds a_t
            sn.cstep = se->step0 + t;
            sn.step = t;
            sn.slot0 = t % (lat + 1);
            hipLaunchKernelGGL(ftmpc::ftmpc_sense_kernel, per_vehicle, wave, 0, s, h->dc, sn);
            HIP_TRY(h, hipGetLastError());
        }
        if (oge.on) {     // availability, outliers into y_t, the availability word for the diagnosis' and the filter's phase 0
            oge.oq.init = t == 0 && !es->xhat;
            oge.oq.cstep = se->step0 + t;
            oge.oq.step = t;
            hipLaunchKernelGGL(ftmpc::ftmpc_outage_kernel, per_vehicle, wave, 0, s, oge.oq);
            HIP_TRY(h, hipGetLastError());
        }
        if (diag) {     // test, decision and re-anchor on y_t; a vehicle that switched has its shifted warm start clipped to the new bounds
            dp.init = t == 0 && !dg->state;
            dp.anchor = (se->step0 + t) % dg->every == 0;
            dp.cstep = (int32_t)(se->step0 + t);
            dp.step = t;
            if (reinstating)     // the rule's test with the hypotheses "listed thruster i is healthy", in place of any phase-0 kernel
                hipLaunchKernelGGL(ftmpc::ftmpc_diagnose_probe_kernel, per_vehicle, wave, 0, s, h->dc, dp, iso.iq, prb.pq,
                                   oge.on ? (const int32_t*)oge.d_avail.p : (const int32_t*)nullptr);
            else if (iso.on)     // the test with the gate, confirmation and revision, in place of either phase-0 kernel
                hipLaunchKernelGGL(ftmpc::ftmpc_diagnose_iso_kernel, per_vehicle, wave, 0, s, h->dc, dp, iso.iq,
                                   oge.on ? (const int32_t*)oge.d_avail.p : (const int32_t*)nullptr);
            else if (oge.on)
                hipLaunchKernelGGL(ftmpc::ftmpc_diagnose_gated_kernel, per_vehicle, wave, 0, s, h->dc, dp, (const int32_t*)oge.d_avail.p);
            else
                hipLaunchKernelGGL(ftmpc::ftmpc_diagnose_kernel<0>, per_vehicle, wave, 0, s, h->dc, dp);
            if (wrench) {     // two launches: the switch kernel's lanes read the offsets the first one wrote
                hw.repair = t > 0 || resume;
                hw.cstep = dp.cstep;
                hipLaunchKernelGGL(ftmpc::ftmpc_hull_offsets_kernel, per_vehicle, wave, 0, s, h->dc, dia.ho);
                hipLaunchKernelGGL(ftmpc::ftmpc_hull_switch_kernel, per_stage, wave, 0, s, h->dc, hw);
            } else if (t > 0 || resume)
                hipLaunchKernelGGL(ftmpc::ftmpc_diagnose_repair_kernel, per_stage, wave, 0, s, B, N, NT, (const int32_t*)dp.switched,
                                   (const double*)h->d_ub, d_warmB);
            HIP_TRY(h, hipGetLastError());
            // a pattern can change at any step without the host knowing: no small grid for a list that was empty the step before
            h->qcnt_valid = false;
            h->qcnt_pending = false;
            if (!sensing && !est)     // nobody else writes the solve's x0: it is the truth
                HIP_TRY(h, hipMemcpyAsync(h->d_x0, sen.d_xtrue, (size_t)B * 13 * sizeof(double), hipMemcpyDeviceToDevice, s));
        }
        if (est) {     // the update on y_t, the estimate (propagated over the queue when the sensor predicts) into h->d_x0
            fp.init = t == 0 && !es->xhat;
            fp.update = (se->step0 + t) % es->every == 0;
            fp.step = t;
            fp.slot0 = t % (lat + 1);
            if (dist) {     // the x pass and the d pass of the augmented update; the d pass writes the solve's x0
                hipLaunchKernelGGL(ftmpc::ftmpc_filter_dist_kernel<0>, per_vehicle, wave, 0, s, h->dc, fp, dst.dq);
                hipLaunchKernelGGL(ftmpc::ftmpc_filter_dist_kernel<1>, per_vehicle, wave, 0, s, h->dc, fp, dst.dq);
            } else if (bias) {     // the x pass in measured coordinates and the bias pass, which completes x^ and writes the solve's x0
                hipLaunchKernelGGL(ftmpc::ftmpc_filter_bias_kernel<0>, per_vehicle, wave, 0, s, h->dc, fp, bia.bq);
                hipLaunchKernelGGL(ftmpc::ftmpc_filter_bias_kernel<1>, per_vehicle, wave, 0, s, h->dc, fp, bia.bq);
            } else if (oge.on)     // (an outage excludes both estimates)
                hipLaunchKernelGGL(ftmpc::ftmpc_filter_gated_kernel, per_vehicle, wave, 0, s, h->dc, fp, oge.gq);
            else
                hipLaunchKernelGGL(ftmpc::ftmpc_filter_kernel<0>, per_vehicle, wave, 0, s, h->dc, fp);
            HIP_TRY(h, hipGetLastError());
        }
        const int64_t xr_s = windows ? xw : 0, ur_s = windows ? uw : 0;
        double* const warm = (t > 0 || resume) ? (wrench ? h->d_warmG.p : d_warmB) : nullptr;
        const double* Ufin = h->d_U;
        const double* Gfin = h->d_G;
        // d^_{t|t} into every linearisation and cost launch of this step's solve (the thruster SQP is refused with an estimate)
        h->lin_dist = dist && db->compensate && !(sqp_iters > 0 && !wrench) ? d_dest : nullptr;
        if (wrench && sqp_iters > 0) {     // the two-stage structure with the nonlinear program of this step solved by the wrench SQP
            ftmpc::SqpState S;
            rc = sqpw_enqueue(h, B, c.hull_rows, has_set, xr_t, xr_s, ur_t, ur_s, warm, sqp_iters, backtracks, c.tol, c.penalty, false, S);
            if (rc == FTMPC_OK) {
                Gfin = S.U;
                sp.status = S.status;
            }
        } else if (sqp_iters > 0) {     // the nonlinear program of this step by the line-search SQP, started from the shifted previous solution
            ftmpc::SqpState S;
            double* J0 = nullptr;
            rc = sqp_enqueue(h, B, xr_t, xr_s, ur_t, ur_s, warm, sqp_iters, backtracks, c.tol, S, &J0);
            if (rc == FTMPC_OK) {
                Ufin = S.U;
                sp.status = S.status;
                HIP_TRY(h, hipMemcpy2DAsync(h->d_u0, NT * sizeof(double), S.U, (size_t)N * NT * sizeof(double), NT * sizeof(double), (size_t)B,
                                         hipMemcpyDeviceToDevice, s));
            }
        } else if (wrench) {         // the reference's two-stage structure: wrench MPC with the hull rows, then allocation
            rc = wrench_enqueue(h, B, c.hull_rows, has_set, xr_t, xr_s, ur_t, ur_s, warm);
        } else {
            rc = enqueue(h, B, h->d_x0, h->d_ub, h->d_stuck, xr_t, xr_s, ur_t, ur_s, warm, h->d_u0, h->d_U, h->d_status, h->d_iters, s, -1);
        }
        h->lin_dist = nullptr;
        if (rc != FTMPC_OK) return rc;
        if (wrench && run.d_abad)
            hipLaunchKernelGGL(ftmpc::ftmpc_count_nonzero_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, B,
                               (const int32_t*)h->d_ast2, run.d_abad + t);
        if (prb.on) {     // at most one quiet thruster per vehicle is pulsed in u_t, before the command enters the ring
            prb.pq.step = t;
            hipLaunchKernelGGL(ftmpc::ftmpc_probe_kernel<0>, per_vehicle, wave, 0, s, h->dc, prb.pq);
        }
        if (lat > 0) {     // u_t waits lat steps: into the slot behind the newest; the plant and the outcomes get the slot of a_t
            HIP_TRY(h, hipMemcpyAsync(d_ring + (size_t)((t + lat) % (lat + 1)) * nu, h->d_u0, nu * sizeof(double), hipMemcpyDeviceToDevice, s));
            sp.u0 = op.u0 = d_ring + (size_t)(t % (lat + 1)) * nu;
        }
        sp.step = t;
        if (env.on) {     // w_c into the plant's force and torque; the estimate's error against it while d^ is the one the solve saw
            env.eq.init = t == 0 && !c.ev->state;
            env.eq.cstep = c.ev->step0 + t;
            env.eq.step = t;
            hipLaunchKernelGGL(ftmpc::ftmpc_environment_kernel, per_vehicle, wave, 0, s, env.eq);
        }
        if (act.on)
            hipLaunchKernelGGL(ftmpc::ftmpc_plant_step_act_kernel, per_vehicle, wave, 0, s, h->dc, sp, pla.pv, act.ap);
        else if (pla.var)
            hipLaunchKernelGGL(ftmpc::ftmpc_plant_step_var_kernel, per_vehicle, wave, 0, s, h->dc, sp, pla.pv);
        else
            hipLaunchKernelGGL(ftmpc::ftmpc_plant_step_kernel, per_vehicle, wave, 0, s, h->dc, sp);
        if (est) {     // the time update under a_t and the controller's pattern of this step
            fp.u = sp.u0;
            if (dist) {     // P_xx, then P_xd, P_dd, the cross terms of P_xx and the mean
                hipLaunchKernelGGL(ftmpc::ftmpc_filter_dist_kernel<2>, per_vehicle, wave, 0, s, h->dc, fp, dst.dq);
                hipLaunchKernelGGL(ftmpc::ftmpc_filter_dist_kernel<3>, per_vehicle, wave, 0, s, h->dc, fp, dst.dq);
            } else if (bias) {     // P_mm, then P_mb, P_bb, the cross terms of P_mm and the mean
                hipLaunchKernelGGL(ftmpc::ftmpc_filter_bias_kernel<2>, per_vehicle, wave, 0, s, h->dc, fp, bia.bq);
                hipLaunchKernelGGL(ftmpc::ftmpc_filter_bias_kernel<3>, per_vehicle, wave, 0, s, h->dc, fp, bia.bq);
            } else
                hipLaunchKernelGGL(ftmpc::ftmpc_filter_kernel<1>, per_vehicle, wave, 0, s, h->dc, fp);
        }
        if (diag) {     // the model's step under a_t and the controller's pattern of this step (with the estimate: d^_{t|t})
            dp.u = sp.u0;
            if (dist)
                hipLaunchKernelGGL(ftmpc::ftmpc_diagnose_dist_kernel, per_vehicle, wave, 0, s, h->dc, dp, (const double*)d_dest);
            else
                hipLaunchKernelGGL(ftmpc::ftmpc_diagnose_kernel<1>, per_vehicle, wave, 0, s, h->dc, dp);
            if (reinstating) {     // a_t of the listed thrusters, which the model's acc leaves out
                prb.pq.u = sp.u0;
                hipLaunchKernelGGL(ftmpc::ftmpc_probe_kernel<1>, per_vehicle, wave, 0, s, h->dc, prb.pq);
            }
        }
        if (out.on) {     // the plant's pattern and the status the plant kernel read; x_{t+1} against column t + 1 of the reference
            op.step = t;
            op.ub = sp.ub;
            op.stuck = sp.stuck;
            op.status = sp.status;
            if (windows || want_cost) {     // a column per vehicle (column 1 of its window, column 0 of its uref window) and / or the cost
                mo.xref = xo_t + 9;
                mo.xref_stride = xr_s;
                mo.uref = uo_t;
                mo.uref_stride = ur_s;
                hipLaunchKernelGGL(ftmpc::ftmpc_outcome_mission_kernel, per_vehicle, wave, 0, s, h->dc, op, mo);
            } else {
                op.xref = run.d_xr + (int64_t)9 * (t + 1);
                hipLaunchKernelGGL(ftmpc::ftmpc_outcome_kernel, per_vehicle, wave, 0, s, h->dc, op);
            }
        }
        if (wrench)     // wrench warm start: shifted by one stage, the last stage repeats
            hipLaunchKernelGGL(ftmpc::ftmpc_shift_warm_kernel, dim3((unsigned)((B * N * 6 + 255) / 256)), dim3(256), 0, s, B, N, 6,
                               Gfin, h->d_warmG, 1);
        else
            hipLaunchKernelGGL(ftmpc::ftmpc_shift_warm_kernel, dim3((unsigned)((B * N * NT + 255) / 256)), dim3(256), 0, s, B, N, NT, Ufin, d_warmB, 0);
        HIP_TRY(h, hipGetLastError());
    }

    // ---- read-backs, one synchronise, the host conversions
    HIP_TRY(h, hipMemcpyAsync(c.x, d_truth, (size_t)B * 13 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (sense) {     // what a continued run resumes from
        if ((rc = h->d_keep_warm.ensure(h, nkeep)) != FTMPC_OK) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->d_keep_warm, wrench ? h->d_warmG.p : d_warmB, (size_t)nkeep * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    LOOP_TRY(sen.fetch(q, se));
    LOOP_TRY(fil.fetch(q, es));
    LOOP_TRY(dst.fetch(q, db));
    LOOP_TRY(bia.fetch(q, c.be));
    LOOP_TRY(oge.fetch(q, c.og));
    LOOP_TRY(env.fetch(q, c.ev));
    LOOP_TRY(iso.fetch(q, c.is));
    LOOP_TRY(prb.fetch(q, c.pb));
    LOOP_TRY(dia.fetch(q, dg, c));
    LOOP_TRY(run.fetch(q, c));
    LOOP_TRY(mis.fetch(q, c.ms, want_cost));
    LOOP_TRY(out.fetch(q, c.oc));
    LOOP_TRY(act.fetch(q, c.ac));
    HIP_TRY(h, hipStreamSynchronize(s));
    act.unpack(q, c.ac);
    dia.unpack(q, dg);
    prb.unpack(q, c.pb);
    dst.unpack(q, db);
    bia.unpack(q, c.be);
    env.unpack(q, c.ev);
    fil.unpack(q, es);
    sen.unpack(q, se);
    if (sense) {
        try {
            h->keep_x.assign(c.x, c.x + B * 13);
            h->keep_B = B;
            h->keep_wrench = wrench;
            h->keep_step = se->step0 + T;
        } catch (const std::bad_alloc&) {
            h->keep_step = -1;      // nothing kept: the next call starts cold
        }
    }
    return FTMPC_OK;
}

// ---- the path of the two widest entries (and of every shard of the multi-GPU driver): checks, the empty run, room on the handle, the loop

void loop_call_features(LoopCall& c, double* x_hist, const ftmpc_fault_schedule* fs, const ftmpc_outcomes* oc, const ftmpc_plant_model* pm,
                        const ftmpc_mission* ms, const ftmpc_actuator* ac, const ftmpc_sensor* se, const ftmpc_estimator* es,
                        const ftmpc_diagnosis* dg, const ftmpc_disturbance* db, const ftmpc_bias_estimate* be,
                        const ftmpc_outage* og = nullptr, const ftmpc_environment* ev = nullptr,
                        const ftmpc_isolation* is = nullptr, const ftmpc_probe* pb = nullptr) {
    c.pb = pb;
    c.x_hist = x_hist;
    c.fs = fs, c.oc = oc, c.pm = pm, c.ms = ms, c.ac = ac, c.se = se, c.es = es, c.dg = dg, c.db = db, c.be = be, c.og = og, c.ev = ev, c.is = is;
}

// the argument checks, in the order the entries have always made them (a bad call keeps its message)
int loop_check(ftmpc_handle* h, const LoopCall& c) {
    const int64_t B = c.B;
    int rc;
    if (c.wrench) {
        if ((rc = sqpw_check(h, c.sqp_iters, c.backtracks, c.tol, c.penalty, c.sqp_iters > 0)) != FTMPC_OK) return rc;
    } else if (c.sqp_iters < 0 || (c.sqp_iters > 0 && (c.backtracks < 1 || !(c.tol >= 0))))
        return fail(h, FTMPC_ERR_ARG, "bad SQP iteration counts");
    if (B < 0 || c.T < 0 || !c.x || !c.ub || !c.stuck || !c.noise || (c.wrench && (!c.hull_A || !c.hull_b)))
        return fail(h, FTMPC_ERR_ARG, "null buffer or negative size");
    const bool own_hull = c.wrench && !c.dg;      // the schedule carries hull tables; under a diagnosis it moves the plant only
    std::string msg;
    if (c.wrench && c.dg && !(msg = wrench_diagnosis_problem(c.fs, c.no_hull_step, B)).empty()) return fail(h, FTMPC_ERR_ARG, msg);
    if ((rc = check_schedule(h, B, c.fs, own_hull, own_hull ? c.n_sets : 0, own_hull && c.hull_set != nullptr)) != FTMPC_OK) return rc;
    if ((rc = check_outcomes(h, B, c.oc, c.wrench)) != FTMPC_OK) return rc;
    if ((rc = check_plant(h, B, c.pm)) != FTMPC_OK) return rc;
    if ((rc = check_sensor(h, B, c.se)) != FTMPC_OK) return rc;
    if ((rc = check_estimator(h, B, c.es)) != FTMPC_OK) return rc;
    if ((rc = check_mission(h, B, c.T, c.ms, c.xref_traj, c.uref_traj, sensor_shift(c.se))) != FTMPC_OK) return rc;
    if ((rc = check_actuator(h, B, c.ac)) != FTMPC_OK) return rc;
    const bool reinstating = probe_reinstates(c.pb);      // widens the detect_level and lead checks
    if (!(msg = diagnosis_problem(c.dg, B, h->cfg.NT, c.es, c.fs, c.se, 0, reinstating)).empty()) return fail(h, FTMPC_ERR_ARG, msg);
    // (the thruster SQP does not know a disturbance estimate; the wrench SQP's cost kernel does: sqp_iters > 0 is served there)
    if (!(msg = disturbance_problem(c.db, B, c.es, c.wrench ? 0 : c.sqp_iters)).empty()) return fail(h, FTMPC_ERR_ARG, msg);
    // (a bias estimate reaches the solve through x0 alone: sqp_iters >= 0 is served)
    if (!(msg = bias_problem(c.be, B, c.es, c.db)).empty()) return fail(h, FTMPC_ERR_ARG, msg);
    if (!(msg = outage_problem(c.og, B, c.es, c.db, c.be)).empty()) return fail(h, FTMPC_ERR_ARG, msg);
    if (!(msg = environment_problem(c.ev, B, c.se, c.db)).empty()) return fail(h, FTMPC_ERR_ARG, msg);
    if (!(msg = isolation_problem(c.is, B, h->cfg.NT, c.dg, 0, reinstating)).empty()) return fail(h, FTMPC_ERR_ARG, msg);
    if (!(msg = probe_problem(c.pb, B, h->cfg.NT, c.dg)).empty()) return fail(h, FTMPC_ERR_ARG, msg);
    return FTMPC_OK;
}

// what a call with B == 0 or T == 0 leaves in its outputs: zero sums, the patterns and offsets it was given
void loop_empty(const LoopCall& c, int NT) {
    const int64_t B = c.B;
    zero_mission_cost(c.ms, B);
    zero_actuator_sums(c.ac, B);
    if (c.es && c.es->err_sq && B > 0) std::fill(c.es->err_sq, c.es->err_sq + B * 4, 0.0);
    if (c.dg && c.dg->ub && B > 0) std::copy(c.ub, c.ub + B * NT, c.dg->ub);
    if (c.dg && c.dg->stuck && B > 0) std::copy(c.stuck, c.stuck + B * NT, c.dg->stuck);
    if (c.wrench && c.out_hull_b && B > 0 && c.hull_rows > 0) std::copy(c.hull_b, c.hull_b + B * c.hull_rows, c.out_hull_b);
}

int loop_run(ftmpc_handle* h, const LoopCall& call) {
    if (check_bias_size(h, call.be) != FTMPC_OK) return FTMPC_ERR_ARG;
    if (!h) return FTMPC_ERR_ARG;
    int rc = loop_check(h, call);
    if (rc != FTMPC_OK) return rc;
    if (call.B == 0 || call.T == 0) {
        loop_empty(call, h->cfg.NT);
        return FTMPC_OK;
    }
    LoopCall c = call;
    if (c.wrench) {
        if ((rc = wrench_prepare(h, c.B, c.hull_A, c.n_sets, c.hull_set, c.hull_b, c.hull_rows)) != FTMPC_OK) return rc;
        const bool sqp = c.sqp_iters > 0;      // without the SQP its settings are not looked at
        c.backtracks = sqp ? c.backtracks : 0;
        c.tol = sqp ? c.tol : 0.0;
        c.penalty = sqp ? (c.penalty > 0 ? c.penalty : FTMPC_SQPW_PENALTY) : 0.0;
    } else {
        HIP_TRY(h, hipSetDevice(h->device));
        if ((rc = ftmpc_reserve(h, c.B)) != FTMPC_OK) return rc;
    }
    return simulate_core(h, c);
}

}  // namespace

extern "C" {

int ftmpc_simulate_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                         const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                         double* u_hist, int32_t* not_converged) {
    return ftmpc_simulate_batch_ex(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, 0, 0, 0.0, u_hist, not_converged);
}

int ftmpc_simulate_faults_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                double* u_hist, double* x_hist, int32_t* not_converged) {
    return ftmpc_simulate_outcomes_batch(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults, u_hist,
                                         x_hist, not_converged, nullptr);
}

int ftmpc_simulate_outcomes_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                  const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                  int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                  double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out) {
    return ftmpc_simulate_plant_batch(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults, u_hist,
                                      x_hist, not_converged, out, nullptr);
}

int ftmpc_simulate_plant_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                               const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                               int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                               double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                               const ftmpc_plant_model* plant) {
    return ftmpc_simulate_mission_batch(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults, u_hist,
                                        x_hist, not_converged, out, plant, nullptr);
}

int ftmpc_simulate_mission_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                 const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                 int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                 double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                 const ftmpc_plant_model* plant, const ftmpc_mission* mission) {
    return ftmpc_simulate_actuator_batch(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults, u_hist,
                                         x_hist, not_converged, out, plant, mission, nullptr);
}

int ftmpc_simulate_actuator_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                  const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                  int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                  double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                  const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator) {
    return ftmpc_simulate_sensor_batch(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults, u_hist,
                                       x_hist, not_converged, out, plant, mission, actuator, nullptr);
}

int ftmpc_simulate_sensor_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                const ftmpc_sensor* sensor) {
    return ftmpc_simulate_estimator_batch(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults, u_hist,
                                          x_hist, not_converged, out, plant, mission, actuator, sensor, nullptr);
}

int ftmpc_simulate_estimator_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                   const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                   int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                   double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                   const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                   const ftmpc_sensor* sensor, const ftmpc_estimator* estimator) {
    return ftmpc_simulate_diagnosis_batch(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults, u_hist,
                                          x_hist, not_converged, out, plant, mission, actuator, sensor, estimator, nullptr);
}

int ftmpc_simulate_diagnosis_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                   const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                   int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                   double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                   const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                   const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis) {
    return ftmpc_simulate_disturbance_batch(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults, u_hist,
                                            x_hist, not_converged, out, plant, mission, actuator, sensor, estimator, diagnosis, nullptr);
}

int ftmpc_simulate_disturbance_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                     const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                     int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                     double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                     const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                     const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                     const ftmpc_disturbance* disturbance) {
    return ftmpc_simulate_bias_batch(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults, u_hist,
                                     x_hist, not_converged, out, plant, mission, actuator, sensor, estimator, diagnosis, disturbance, nullptr);
}

int ftmpc_simulate_bias_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                              const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                              int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                              double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                              const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                              const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                              const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate) {
    return ftmpc_simulate_outage_batch(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults, u_hist,
                                       x_hist, not_converged, out, plant, mission, actuator, sensor, estimator, diagnosis, disturbance,
                                       bias_estimate, nullptr);
}

int ftmpc_simulate_outage_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                                const ftmpc_outage* outage) {
    return ftmpc_simulate_environment_batch(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults,
                                            u_hist, x_hist, not_converged, out, plant, mission, actuator, sensor, estimator, diagnosis,
                                            disturbance, bias_estimate, outage, nullptr);
}

int ftmpc_simulate_environment_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                     const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                     int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                     double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                     const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                     const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                     const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                                     const ftmpc_outage* outage, const ftmpc_environment* environment) {
    return ftmpc_simulate_isolation_batch(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults,
                                          u_hist, x_hist, not_converged, out, plant, mission, actuator, sensor, estimator, diagnosis,
                                          disturbance, bias_estimate, outage, environment, nullptr);
}

int ftmpc_simulate_isolation_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                   const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                   int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                                   double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                                   const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                                   const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                                   const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                                   const ftmpc_outage* outage, const ftmpc_environment* environment,
                                   const ftmpc_isolation* isolation) {
    return ftmpc_simulate_probe_batch(h, B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, faults, u_hist,
                                      x_hist, not_converged, out, plant, mission, actuator, sensor, estimator, diagnosis, disturbance,
                                      bias_estimate, outage, environment, isolation, nullptr);
}

int ftmpc_simulate_probe_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                               const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                               int32_t sqp_iters, int32_t backtracks, double tol, const ftmpc_fault_schedule* faults,
                               double* u_hist, double* x_hist, int32_t* not_converged, const ftmpc_outcomes* out,
                               const ftmpc_plant_model* plant, const ftmpc_mission* mission, const ftmpc_actuator* actuator,
                               const ftmpc_sensor* sensor, const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis,
                               const ftmpc_disturbance* disturbance, const ftmpc_bias_estimate* bias_estimate,
                               const ftmpc_outage* outage, const ftmpc_environment* environment,
                               const ftmpc_isolation* isolation, const ftmpc_probe* probe) {
    LoopCall c = loop_call(B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, u_hist, not_converged);
    loop_call_features(c, x_hist, faults, out, plant, mission, actuator, sensor, estimator, diagnosis, disturbance, bias_estimate, outage,
                       environment, isolation, probe);
    return loop_run(h, c);
}

int ftmpc_simulate_wrench_faults_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                       const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                       const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                       int32_t sqp_iters, int32_t backtracks, double tol, double penalty, const ftmpc_fault_schedule* faults,
                                       double* u_hist, double* x_hist, int32_t* not_converged, int32_t* alloc_failed) {
    return ftmpc_simulate_wrench_outcomes_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj, noise,
                                                seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged, alloc_failed,
                                                nullptr);
}

int ftmpc_simulate_wrench_outcomes_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                         const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                         const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                         int32_t sqp_iters, int32_t backtracks, double tol, double penalty, const ftmpc_fault_schedule* faults,
                                         double* u_hist, double* x_hist, int32_t* not_converged, int32_t* alloc_failed,
                                         const ftmpc_outcomes* out) {
    return ftmpc_simulate_wrench_plant_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj, noise,
                                             seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged, alloc_failed,
                                             out, nullptr);
}

int ftmpc_simulate_wrench_plant_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                      const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                      const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                      int32_t sqp_iters, int32_t backtracks, double tol, double penalty, const ftmpc_fault_schedule* faults,
                                      double* u_hist, double* x_hist, int32_t* not_converged, int32_t* alloc_failed,
                                      const ftmpc_outcomes* out, const ftmpc_plant_model* plant) {
    return ftmpc_simulate_wrench_mission_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj, noise,
                                               seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged, alloc_failed,
                                               out, plant, nullptr);
}

int ftmpc_simulate_wrench_mission_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                        const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                        const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                        int32_t sqp_iters, int32_t backtracks, double tol, double penalty, const ftmpc_fault_schedule* faults,
                                        double* u_hist, double* x_hist, int32_t* not_converged, int32_t* alloc_failed,
                                        const ftmpc_outcomes* out, const ftmpc_plant_model* plant, const ftmpc_mission* mission) {
    return ftmpc_simulate_wrench_actuator_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj, noise,
                                                seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged, alloc_failed,
                                                out, plant, mission, nullptr);
}

int ftmpc_simulate_wrench_actuator_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                         const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                         const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                         int32_t sqp_iters, int32_t backtracks, double tol, double penalty, const ftmpc_fault_schedule* faults,
                                         double* u_hist, double* x_hist, int32_t* not_converged, int32_t* alloc_failed,
                                         const ftmpc_outcomes* out, const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                         const ftmpc_actuator* actuator) {
    return ftmpc_simulate_wrench_sensor_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj, noise,
                                              seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged, alloc_failed,
                                              out, plant, mission, actuator, nullptr);
}

int ftmpc_simulate_wrench_sensor_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                       const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                       const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                       int32_t sqp_iters, int32_t backtracks, double tol, double penalty, const ftmpc_fault_schedule* faults,
                                       double* u_hist, double* x_hist, int32_t* not_converged, int32_t* alloc_failed,
                                       const ftmpc_outcomes* out, const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                       const ftmpc_actuator* actuator, const ftmpc_sensor* sensor) {
    return ftmpc_simulate_wrench_estimator_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj, noise,
                                                 seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged, alloc_failed,
                                                 out, plant, mission, actuator, sensor, nullptr);
}

int ftmpc_simulate_wrench_estimator_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                          const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                          int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                          uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                          const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist, int32_t* not_converged,
                                          int32_t* alloc_failed, const ftmpc_outcomes* out, const ftmpc_plant_model* plant,
                                          const ftmpc_mission* mission, const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                          const ftmpc_estimator* estimator) {
    return ftmpc_simulate_wrench_diagnosis_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj, noise,
                                                 seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged, alloc_failed,
                                                 out, plant, mission, actuator, sensor, estimator, nullptr, nullptr, nullptr);
}

int ftmpc_simulate_wrench_diagnosis_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                          const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                          int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                          uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                          const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist, int32_t* not_converged,
                                          int32_t* alloc_failed, const ftmpc_outcomes* out, const ftmpc_plant_model* plant,
                                          const ftmpc_mission* mission, const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                          const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                          int32_t* no_hull_step) {
    return ftmpc_simulate_wrench_disturbance_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj,
                                                   noise, seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged,
                                                   alloc_failed, out, plant, mission, actuator, sensor, estimator, diagnosis, out_hull_b,
                                                   no_hull_step, nullptr);
}

int ftmpc_simulate_wrench_disturbance_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                            const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                            int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                            uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                            const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist, int32_t* not_converged,
                                            int32_t* alloc_failed, const ftmpc_outcomes* out, const ftmpc_plant_model* plant,
                                            const ftmpc_mission* mission, const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                            const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                            int32_t* no_hull_step, const ftmpc_disturbance* disturbance) {
    return ftmpc_simulate_wrench_bias_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj, noise,
                                            seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged, alloc_failed,
                                            out, plant, mission, actuator, sensor, estimator, diagnosis, out_hull_b, no_hull_step,
                                            disturbance, nullptr);
}

int ftmpc_simulate_wrench_bias_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                     const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                     int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                     uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                     const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist, int32_t* not_converged,
                                     int32_t* alloc_failed, const ftmpc_outcomes* out, const ftmpc_plant_model* plant,
                                     const ftmpc_mission* mission, const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                     const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                     int32_t* no_hull_step, const ftmpc_disturbance* disturbance,
                                     const ftmpc_bias_estimate* bias_estimate) {
    return ftmpc_simulate_wrench_outage_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj, noise,
                                              seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged, alloc_failed,
                                              out, plant, mission, actuator, sensor, estimator, diagnosis, out_hull_b, no_hull_step,
                                              disturbance, bias_estimate, nullptr);
}

int ftmpc_simulate_wrench_outage_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                       const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                       int32_t hull_rows, const double* xref_traj, const double* uref_traj, const double noise[4],
                                       uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                       const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist, int32_t* not_converged,
                                       int32_t* alloc_failed, const ftmpc_outcomes* out, const ftmpc_plant_model* plant,
                                       const ftmpc_mission* mission, const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                       const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                       int32_t* no_hull_step, const ftmpc_disturbance* disturbance,
                                       const ftmpc_bias_estimate* bias_estimate, const ftmpc_outage* outage) {
    return ftmpc_simulate_wrench_environment_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj,
                                                   noise, seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged,
                                                   alloc_failed, out, plant, mission, actuator, sensor, estimator, diagnosis, out_hull_b,
                                                   no_hull_step, disturbance, bias_estimate, outage, nullptr);
}

int ftmpc_simulate_wrench_environment_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                            const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                            int32_t hull_rows, const double* xref_traj, const double* uref_traj,
                                            const double noise[4], uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol,
                                            double penalty, const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                            int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                            const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                            const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                            const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                            int32_t* no_hull_step, const ftmpc_disturbance* disturbance,
                                            const ftmpc_bias_estimate* bias_estimate, const ftmpc_outage* outage,
                                            const ftmpc_environment* environment) {
    return ftmpc_simulate_wrench_isolation_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj,
                                                 noise, seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged,
                                                 alloc_failed, out, plant, mission, actuator, sensor, estimator, diagnosis, out_hull_b,
                                                 no_hull_step, disturbance, bias_estimate, outage, environment, nullptr);
}

int ftmpc_simulate_wrench_isolation_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                          const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                          int32_t hull_rows, const double* xref_traj, const double* uref_traj,
                                          const double noise[4], uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol,
                                          double penalty, const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                          int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                          const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                          const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                          const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                          int32_t* no_hull_step, const ftmpc_disturbance* disturbance,
                                          const ftmpc_bias_estimate* bias_estimate, const ftmpc_outage* outage,
                                          const ftmpc_environment* environment, const ftmpc_isolation* isolation) {
    return ftmpc_simulate_wrench_probe_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj,
                                             noise, seed, sqp_iters, backtracks, tol, penalty, faults, u_hist, x_hist, not_converged,
                                             alloc_failed, out, plant, mission, actuator, sensor, estimator, diagnosis, out_hull_b,
                                             no_hull_step, disturbance, bias_estimate, outage, environment, isolation, nullptr);
}

int ftmpc_simulate_wrench_probe_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                      const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b,
                                      int32_t hull_rows, const double* xref_traj, const double* uref_traj,
                                      const double noise[4], uint64_t seed, int32_t sqp_iters, int32_t backtracks, double tol,
                                      double penalty, const ftmpc_fault_schedule* faults, double* u_hist, double* x_hist,
                                      int32_t* not_converged, int32_t* alloc_failed, const ftmpc_outcomes* out,
                                      const ftmpc_plant_model* plant, const ftmpc_mission* mission,
                                      const ftmpc_actuator* actuator, const ftmpc_sensor* sensor,
                                      const ftmpc_estimator* estimator, const ftmpc_diagnosis* diagnosis, double* out_hull_b,
                                      int32_t* no_hull_step, const ftmpc_disturbance* disturbance,
                                      const ftmpc_bias_estimate* bias_estimate, const ftmpc_outage* outage,
                                      const ftmpc_environment* environment, const ftmpc_isolation* isolation,
                                      const ftmpc_probe* probe) {
    LoopCall c = loop_call(B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, u_hist, not_converged);
    loop_call_wrench(c, hull_A, n_sets, hull_set, hull_b, hull_rows, penalty, alloc_failed);
    c.out_hull_b = out_hull_b;
    c.no_hull_step = no_hull_step;
    loop_call_features(c, x_hist, faults, out, plant, mission, actuator, sensor, estimator, diagnosis, disturbance, bias_estimate, outage,
                       environment, isolation, probe);
    return loop_run(h, c);
}

// The three narrow entries keep their own, narrower checks (no feature struct reaches them).

int ftmpc_simulate_batch_ex(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                            const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                            int32_t sqp_iters, int32_t backtracks, double tol, double* u_hist, int32_t* not_converged) {
    if (!h) return FTMPC_ERR_ARG;
    if (sqp_iters < 0 || (sqp_iters > 0 && (backtracks < 1 || !(tol >= 0)))) return fail(h, FTMPC_ERR_ARG, "bad SQP iteration counts");
    if (B < 0 || T < 0 || !x || !ub || !stuck || !xref_traj || !noise) return fail(h, FTMPC_ERR_ARG, "null buffer or negative size");
    if (B == 0 || T == 0) return FTMPC_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ftmpc_reserve(h, B);
    if (rc != FTMPC_OK) return rc;
    return simulate_core(h, loop_call(B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, u_hist, not_converged));
}

int ftmpc_simulate_wrench_batch(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                double* u_hist, int32_t* not_converged, int32_t* alloc_failed) {
    if (!h) return FTMPC_ERR_ARG;
    if (B < 0 || T < 0 || !x || !ub || !stuck || !xref_traj || !noise || !hull_A || !hull_b) return fail(h, FTMPC_ERR_ARG, "null buffer or negative size");
    if (B == 0 || T == 0) return FTMPC_OK;
    int rc = wrench_prepare(h, B, hull_A, n_sets, hull_set, hull_b, hull_rows);
    if (rc != FTMPC_OK) return rc;
    LoopCall c = loop_call(B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, 0, 0, 0.0, u_hist, not_converged);
    loop_call_wrench(c, hull_A, n_sets, hull_set, hull_b, hull_rows, 0.0, alloc_failed);
    return simulate_core(h, c);
}

int ftmpc_simulate_wrench_batch_ex(ftmpc_handle* h, int64_t B, int32_t T, double* x, const double* ub, const double* stuck,
                                   const double* hull_A, int32_t n_sets, const int32_t* hull_set, const double* hull_b, int32_t hull_rows,
                                   const double* xref_traj, const double* uref_traj, const double noise[4], uint64_t seed,
                                   int32_t sqp_iters, int32_t backtracks, double tol, double penalty,
                                   double* u_hist, int32_t* not_converged, int32_t* alloc_failed) {
    if (!h) return FTMPC_ERR_ARG;
    int rc = sqpw_check(h, sqp_iters, backtracks, tol, penalty, sqp_iters > 0);
    if (rc != FTMPC_OK) return rc;
    if (sqp_iters == 0)
        return ftmpc_simulate_wrench_batch(h, B, T, x, ub, stuck, hull_A, n_sets, hull_set, hull_b, hull_rows, xref_traj, uref_traj, noise,
                                           seed, u_hist, not_converged, alloc_failed);
    if (B < 0 || T < 0 || !x || !ub || !stuck || !xref_traj || !noise || !hull_A || !hull_b) return fail(h, FTMPC_ERR_ARG, "null buffer or negative size");
    if (B == 0 || T == 0) return FTMPC_OK;
    if ((rc = wrench_prepare(h, B, hull_A, n_sets, hull_set, hull_b, hull_rows)) != FTMPC_OK) return rc;
    LoopCall c = loop_call(B, T, x, ub, stuck, xref_traj, uref_traj, noise, seed, sqp_iters, backtracks, tol, u_hist, not_converged);
    loop_call_wrench(c, hull_A, n_sets, hull_set, hull_b, hull_rows, penalty > 0 ? penalty : FTMPC_SQPW_PENALTY, alloc_failed);
    return simulate_core(h, c);
}

}  // extern "C"
