// jf_engine_cone.cpp -- the host side of object poses, following listeners and talker cones (include/jefferson.h: "talker cones
// and heads that follow objects").  The setters (jf_object_set_pose, jf_listener_follow_object,
// jf_object_set_cone) only write host state under the positions' mutex.  A followed object's pose IS its bus's pose wherever
// the host resolves one (listener_pose: the per-block snapshot, jf_listener_get_pose); the objects batch calls resolve it on the
// device (pose_follow_kernel, launched by jf_engine.cpp's upload).  The cone is the eighth latched control: a processing call
// latches it inside gate_latch (cone_latch_host under that mutex, cone_latch_active behind the gates' own buffers), and
// run_gate_stage launches cone_gain_kernel (jf_cone.hip) behind the range stage and ahead of the voice limits, the levellers and
// desc_gain_kernel (run_cone_stage).  jf_cone_gain and jf_debug_cone_scan are the rule on the host -- the header the kernel
// compiles (jf_cone_rule.h).
//
// Who reads what: object_quat / follow / cn_cone / cn.report.last / .blocks are touched under pos_mu only; cn.on, run_cn*, cn.idle,
// cn_cur and the device buffers belong to the thread that makes the processing calls.  The state {d_prev} is on the device only
// (d_cn_dprev), two planes taken in turn as the hearing range's are (jf_engine_range.cpp).
//
// WHERE A RUN'S POSES LIE (e->call_geo).  0, a per-block call or records given as such: the latched poses, uploaded here
// (d_cn_geo), every stride 0.  1, world positions per source: no source is attached for the call, every d is 1.  2, an objects
// call: the call's positions and listener poses on the device, the orientations latched when the trajectory was uploaded
// (e->traj_ori, the ones its records were formed with where a bus follows) from d_cn_geo.  3, an object-poses call:
// all of it the call's.
#include "jf_engine_internal.h"

static const float kIdentityQuat[4] = {1.0f, 0.0f, 0.0f, 0.0f};
static const float kDefaultCone[kConeFloats] = {360.0f, 360.0f, 1.0f};

const float *object_quat_of(const jf_engine *e, int obj) {  // under pos_mu
    return e->object_quat.empty() ? kIdentityQuat : e->object_quat.data() + 4 * (size_t)obj;
}

int follow_of(const jf_engine *e, int bus) {  // under pos_mu
    return e->follow.empty() || bus < 0 || (size_t)bus >= e->follow.size() ? -1 : e->follow[bus];
}

void listener_pose(const jf_engine *e, int bus, float out[kPoseFloats]) {  // under pos_mu
    const int o = follow_of(e, bus);
    if (o >= 0) {
        std::copy(e->object_world.begin() + 3 * (size_t)o, e->object_world.begin() + 3 * (size_t)o + 3, out);
        std::copy(object_quat_of(e, o), object_quat_of(e, o) + 4, out + 3);
    } else if (e->pose.empty()) {
        out[0] = out[1] = out[2] = out[4] = out[5] = out[6] = 0.0f;
        out[3] = 1.0f;
    } else {
        std::copy(e->pose.begin() + (size_t)kPoseFloats * bus, e->pose.begin() + (size_t)kPoseFloats * (bus + 1), out);
    }
}

bool coned(const jf_engine *e) {  // under pos_mu
    for (size_t o = 0; kConeFloats * o + 2 < e->cn_cone.size(); o++)
        if (!cone_is_default(e->cn_cone[kConeFloats * o], e->cn_cone[kConeFloats * o + 1], e->cn_cone[kConeFloats * o + 2])) return true;
    return false;
}

// under pos_mu: the call's planes, maps and latched poses as the device is to hold them; true while some object has a cone.  A
// call that is latched without one leaves every state at 1: remembered here, carried out by the next latch that is active.
bool cone_latch_host(jf_engine *e) {
    if (!coned(e)) {
        if (e->d_cn_dprev) e->cn.idle = true;
        return false;
    }
    const size_t S = (size_t)e->S, no = (size_t)e->n_objects, nb = (size_t)e->n_buses;
    const bool from_traj = e->call_geo >= 2;  // the maps the trajectory's records were formed with
    e->run_cn.assign(kConeFloats * S, 1.0f);
    e->run_cn_map.assign(3 * S, -1);
    for (size_t s = 0; s < S; s++) {
        int o = -1;
        if (e->call_geo != 1) {
            const std::vector<int> &map = from_traj ? e->object_of_dev : e->object_of;
            o = map.empty() ? -1 : map[s];
        }
        const int b = e->bus.empty() ? 0 : e->bus[s];
        const float *c = o >= 0 && (size_t)o < no && !e->cn_cone.empty() ? e->cn_cone.data() + kConeFloats * (size_t)o : kDefaultCone;
        if (o < 0 || (size_t)o >= no || cone_is_default(c[0], c[1], c[2])) o = -1, c = kDefaultCone;
        e->run_cn[s] = c[0];
        e->run_cn[S + s] = c[1];
        e->run_cn[2 * S + s] = c[2];
        e->run_cn_map[s] = o;
        e->run_cn_map[S + s] = b;
        int fo = from_traj ? (e->traj_follow && !e->follow_src_dev.empty() ? e->follow_src_dev[s] : -1) : follow_of(e, b);
        if (fo >= 0 && (size_t)fo >= no) fo = -1;
        e->run_cn_map[2 * S + s] = fo;
    }
    e->cn_geo_objects = no;
    e->run_cn_geo.assign(7 * no + (size_t)kPoseFloats * nb, 0.0f);
    std::copy(e->object_world.begin(), e->object_world.begin() + 3 * no, e->run_cn_geo.begin());
    // (an objects trajectory: the orientations it was uploaded with -- one moment for its records and its cones, follow or not)
    const bool held = e->call_geo == 2 && e->traj_ori.size() == 4 * no;
    for (size_t o = 0; o < no; o++) {
        const float *q = held ? e->traj_ori.data() + 4 * o : e->call_geo == 2 ? kIdentityQuat : object_quat_of(e, (int)o);
        std::copy(q, q + 4, e->run_cn_geo.begin() + 3 * no + 4 * o);
    }
    for (size_t b = 0; b < nb; b++) listener_pose(e, (int)b, e->run_cn_geo.data() + 7 * no + (size_t)kPoseFloats * b);
    return true;
}

int cone_latch_active(jf_engine *e) {
    const size_t S = (size_t)e->S;
    if (e->call_geo >= 2 && ((size_t)e->traj_n_objects != e->cn_geo_objects || e->traj_n_buses != e->n_buses))
        return fail(e, JF_ERR_STATE, "talker cones: the objects or buses have changed since the trajectory was uploaded");
    if (!e->d_cn_dprev) {
        JF_HIP(e, e->cn.d_par.alloc(kConeFloats * S));
        JF_HIP(e, e->d_cn_map.alloc(3 * S));
        int rc = e->cn.report.alloc(e);
        if (rc) return rc;
        DevBuf<float> st;
        JF_HIP(e, st.alloc(2 * S));
        rc = state_fill(e, st, kOneBits, 2, -1);  // both planes: everybody was heard, in stream order
        if (rc) return rc;
        e->cn.dev.clear();
        e->dev_cn_map.clear();
        e->cn.idle = false;
        e->cn_cur = 0;
        e->d_cn_dprev = std::move(st);
    }
    if (e->cn.idle) {
        const int rc = cone_reset_source(e, -1);
        if (rc) return rc;
        e->cn.idle = false;
    }
    const size_t len = e->run_cn_geo.size();
    if (len != e->cn_geo_len) {  // the counts have changed: the image is laid out anew (rare; what is in line reads the old one)
        JF_HIP(e, hipStreamSynchronize(e->stream));
        e->dev_cn_geo.clear();
        e->cn_geo_len = 0;
        e->d_cn_geo.reset();
        e->cn_geo_ring.reset(new StagedRing<float>());
        JF_HIP(e, e->d_cn_geo.alloc(len));
        e->cn_geo_len = len;
    }
    int rc = staged_upload(e, e->cn.ring, kConeFloats * S, StagedPart<float>{e->cn.d_par, e->cn.dev, e->run_cn, 0, e->cn.dev != e->run_cn});
    if (rc == JF_OK)
        rc = staged_upload(e, e->cn_map_ring, 3 * S, StagedPart<int>{e->d_cn_map, e->dev_cn_map, e->run_cn_map, 0, e->dev_cn_map != e->run_cn_map});
    if (rc == JF_OK)
        rc = staged_upload(e, *e->cn_geo_ring, len, StagedPart<float>{e->d_cn_geo, e->dev_cn_geo, e->run_cn_geo, 0, e->dev_cn_geo != e->run_cn_geo});
    return rc;
}

// Behind the range stage and ahead of the voice stage of this run.  g_eff / g_eff_prev are the gate stage's, rewritten in
// place; d [K][S] is kept for the input meters' copies.
int run_cone_stage(jf_engine *e, float *g_eff, float *g_eff_prev, int K, bool timed) {
    const size_t S = (size_t)e->S, no = e->cn_geo_objects;
    ConeGeometry g = {};
    const float *img = e->d_cn_geo.p;
    if (e->call_geo >= 2) {
        if (e->run_first_block < 0 || !e->traj_dgeo.obj_pos) return fail(e, JF_ERR_STATE, "talker cones: the run has no poses");
        const size_t k0 = (size_t)e->run_first_block;
        g = e->traj_dgeo;
        g.obj_pos += k0 * (size_t)g.pos_stride;
        if (e->call_geo == 3) {
            g.obj_ori += k0 * (size_t)g.ori_stride;
        } else {  // an objects call brings no orientations: the ones latched at its upload, in the image
            g.obj_ori = img + 3 * no;
            g.ori_pitch = 4;
            g.ori_stride = 0;
        }
        if (g.lis) g.lis += k0 * (size_t)g.lis_stride;
    } else {
        g.obj_pos = img;
        g.pos_pitch = 3;
        g.obj_ori = img + 3 * no;
        g.ori_pitch = 4;
        g.lis = img + 7 * no;
    }
    const float *d_in = e->d_cn_dprev.p + (size_t)e->cn_cur * S;
    float *d_to = e->d_cn_dprev.p + (size_t)(e->cn_cur ^ 1) * S;
    int rc = e->cn.tm.begin(e, timed);
    if (rc) return rc;
    JF_HIP(e, launch_cone_gain(g, e->cn.d_par, e->d_cn_map, g_eff, g_eff_prev, d_in, d_to, e->gate_meters ? e->cn.report.d.p : nullptr, e->S, K,
                               e->stream));
    rc = e->cn.tm.end(e, timed);
    if (rc) return rc;
    e->cn_cur ^= 1;  // (the next run, and a reset in between, meet what this one wrote)
    e->cn.last = true;
    return JF_OK;
}

// src < 0: every source.  A source that starts over was heard in full before; the cones stay.  The plane the next run reads.
int cone_reset_source(jf_engine *e, int src) {
    if (!e->d_cn_dprev) return JF_OK;
    return state_fill(e, e->d_cn_dprev.p + (size_t)e->cn_cur * (size_t)e->S, kOneBits, 1, src);
}

// under pos_mu: the objects that remain keep their orientations and cones, new ones face along the identity and have none
void cone_set_objects(jf_engine *e, int n_objects) {
    if (!e->object_quat.empty()) {
        const size_t have = e->object_quat.size();
        e->object_quat.resize(4 * (size_t)n_objects, 0.0f);
        for (size_t i = have; i < e->object_quat.size(); i += 4) e->object_quat[i] = 1.0f;
    }
    if (!e->cn_cone.empty()) {
        const size_t have = e->cn_cone.size();
        e->cn_cone.resize(kConeFloats * (size_t)n_objects, 0.0f);
        for (size_t i = have; i < e->cn_cone.size(); i += kConeFloats) std::copy(kDefaultCone, kDefaultCone + kConeFloats, e->cn_cone.begin() + i);
    }
}

// under pos_mu: the buses that remain keep their follows, new ones follow nothing
void follow_set_buses(jf_engine *e, int n_buses) {
    if (!e->follow.empty()) e->follow.resize((size_t)n_buses, -1);
}

static const char *kConeArgMsg = "cone: all three finite; 0 <= inner <= outer <= 360 degrees, 0 <= outer_gain <= 1";
static const char *kConeReverbMsg = "a talker cone is not offered while a reverb response is set (its wet tail outlives the dry talker)";
static const char *kObjPoseArgMsg = "a non-finite value, or a quaternion whose norm is further than 1e-3 from 1";

extern "C" {

int jf_object_set_pose(jf_engine *e, int obj, const float position[3], const float orientation[4]) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (!position || !orientation) return fail(e, JF_ERR_ARG, "null pose");
    const float p[kPoseFloats] = {position[0], position[1], position[2], orientation[0], orientation[1], orientation[2], orientation[3]};
    if (!pose_valid(p)) return fail(e, JF_ERR_ARG, kObjPoseArgMsg);
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (obj < 0 || obj >= e->n_objects) return fail(e, JF_ERR_ARG, "bad object index");
    const bool identity = p[3] == 1.0f && p[4] == 0.0f && p[5] == 0.0f && p[6] == 0.0f;
    if (e->object_quat.empty() && !identity) {
        e->object_quat.assign(4 * (size_t)e->n_objects, 0.0f);
        for (int o = 0; o < e->n_objects; o++) e->object_quat[4 * (size_t)o] = 1.0f;
    }
    std::copy(p, p + 3, e->object_world.begin() + 3 * (size_t)obj);
    if (!e->object_quat.empty()) std::copy(p + 3, p + kPoseFloats, e->object_quat.begin() + 4 * (size_t)obj);
    return JF_OK;
    });
}

int jf_object_get_pose(const jf_engine *e, int obj, float out[7]) {
    return jf_guard([&]() -> int {
    if (!e || !out) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    if (obj < 0 || obj >= e->n_objects) return JF_ERR_ARG;
    std::copy(e->object_world.begin() + 3 * (size_t)obj, e->object_world.begin() + 3 * (size_t)obj + 3, out);
    std::copy(object_quat_of(e, obj), object_quat_of(e, obj) + 4, out + 3);
    return JF_OK;
    });
}

int jf_listener_follow_object(jf_engine *e, int bus, int obj) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (bus < 0 || bus >= e->n_buses) return fail(e, JF_ERR_ARG, "bad bus index");
    if (obj >= e->n_objects) return fail(e, JF_ERR_ARG, "bad object index");
    if (obj < 0) {  // detach: the bus keeps the pose the object holds now -- nothing jumps
        if (follow_of(e, bus) < 0) return JF_OK;
        float p[kPoseFloats];
        listener_pose(e, bus, p);
        if (e->pose.empty()) {
            e->pose.assign((size_t)kPoseFloats * e->n_buses, 0.0f);
            for (int b = 0; b < e->n_buses; b++) e->pose[(size_t)kPoseFloats * b + 3] = 1.0f;
        }
        std::copy(p, p + kPoseFloats, e->pose.begin() + (size_t)kPoseFloats * bus);
        e->follow[bus] = -1;
        return JF_OK;
    }
    if (e->follow.empty()) e->follow.assign((size_t)e->n_buses, -1);
    e->follow[bus] = obj;
    return JF_OK;
    });
}

int jf_listener_object(const jf_engine *e, int bus) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    if (bus < 0 || bus >= e->n_buses) return JF_ERR_ARG;
    return follow_of(e, bus);
    });
}

int jf_object_set_cone(jf_engine *e, int obj, float inner_deg, float outer_deg, float outer_gain) {
    return jf_guard([&]() -> int {
    if (!e) return JF_ERR_ARG;
    if (!cone_params_ok(inner_deg, outer_deg, outer_gain)) return fail(e, JF_ERR_ARG, kConeArgMsg);
    const bool def = cone_is_default(inner_deg, outer_deg, outer_gain);
    if (!def && e->rv_P > 0) return fail(e, JF_ERR_STATE, kConeReverbMsg);
    std::lock_guard<std::mutex> lk(e->pos_mu);
    if (obj < 0 || obj >= e->n_objects) return fail(e, JF_ERR_ARG, "bad object index");
    if (e->cn_cone.empty() && def) return JF_OK;  // (no object has a cone until one is set)
    if (e->cn_cone.empty()) {
        e->cn_cone.resize(kConeFloats * (size_t)e->n_objects);
        for (int o = 0; o < e->n_objects; o++) std::copy(kDefaultCone, kDefaultCone + kConeFloats, e->cn_cone.begin() + kConeFloats * (size_t)o);
    }
    float *c = e->cn_cone.data() + kConeFloats * (size_t)obj;
    c[0] = inner_deg;
    c[1] = outer_deg;
    c[2] = outer_gain;
    return JF_OK;
    });
}

int jf_object_cone(const jf_engine *e, int obj, float *inner_deg, float *outer_deg, float *outer_gain) {
    return jf_guard([&]() -> int {
    if (!e || !inner_deg || !outer_deg || !outer_gain) return JF_ERR_ARG;
    jf_engine *m = const_cast<jf_engine *>(e);
    std::lock_guard<std::mutex> lk(m->pos_mu);
    if (obj < 0 || obj >= e->n_objects) return JF_ERR_ARG;
    const float *c = e->cn_cone.empty() ? kDefaultCone : e->cn_cone.data() + kConeFloats * (size_t)obj;
    *inner_deg = c[0];
    *outer_deg = c[1];
    *outer_gain = c[2];
    return JF_OK;
    });
}

int jf_source_cone_gains(jf_engine *e, int n_blocks, float *out) {
    if (!e) return JF_ERR_ARG;
    return source_report(e, e->cn.report, coned, "no object has a cone (jf_object_set_cone)",
                         "no call has been rendered with a talker cone and input meters yet", n_blocks, out);
}

// The rule without an engine: d of one talker heard from one head centre.
int jf_cone_gain(float inner_deg, float outer_deg, float outer_gain, const float talker_pose[7], const float listener_centre[3], float *d_out) {
    if (!d_out || !talker_pose || !listener_centre || !cone_params_ok(inner_deg, outer_deg, outer_gain)) return JF_ERR_ARG;
    if (!pose_valid(talker_pose) || !pose_finite(listener_centre[0]) || !pose_finite(listener_centre[1]) || !pose_finite(listener_centre[2]))
        return JF_ERR_ARG;
    *d_out = cone_gain(inner_deg, outer_deg, outer_gain, talker_pose, talker_pose + 3, listener_centre);
    return JF_OK;
}

// The rule on the host: one run of K blocks over S sources.  object_poses [K][n_objects][7], listener_poses [K][n_buses][7];
// par [3][S] inner, outer, outer_gain per source; object_of / bus / follow [S] (-1: none; follow: the object the listener of the
// source's bus follows); *d_prev_io [S] is the state before the run and, on return, after it (K == 0 leaves it).
int jf_debug_cone_scan(const float *object_poses, const float *listener_poses, int n_blocks, int n_sources, int n_objects, int n_buses,
                       const float *par, const int *object_of, const int *bus, const int *follow, float *d_prev_io, float *d_out) {
    const int K = n_blocks, S = n_sources;
    if (K < 0 || S <= 0 || n_objects <= 0 || n_buses <= 0 || !par || !object_of || !bus || !follow || !d_prev_io ||
        (K > 0 && (!object_poses || !listener_poses || !d_out)))
        return JF_ERR_ARG;
    for (int s = 0; s < S; s++) {
        if (!cone_params_ok(par[s], par[(size_t)S + s], par[2 * (size_t)S + s])) return JF_ERR_ARG;
        if (object_of[s] >= n_objects || follow[s] >= n_objects || bus[s] < 0 || bus[s] >= n_buses) return JF_ERR_ARG;
    }
    ConeGeometry g = {};
    g.obj_pos = object_poses;
    g.obj_ori = object_poses ? object_poses + 3 : nullptr;
    g.lis = listener_poses;
    g.pos_pitch = g.ori_pitch = kPoseFloats;
    g.pos_stride = g.ori_stride = kPoseFloats * n_objects;
    g.lis_stride = kPoseFloats * n_buses;
    cone_run(g, K, S, par, object_of, bus, follow, d_prev_io, d_out);
    return JF_OK;
}

// device and pinned memory held for cones: the parameter and map planes, the state's two, a run's d and where it lands, the
// latched poses (the staging rings apart)
long long jf_debug_cone_bytes(const jf_engine *e) {
    if (!e) return JF_ERR_ARG;
    if (!e->d_cn_dprev) return 0;
    const long long S = e->S, KS = (long long)e->maxK * S;
    return (long long)sizeof(float) * (3 * S + 3 * S + 2 * S + KS + KS + (long long)e->cn_geo_len);
}

int jf_profile_read_cone(jf_engine *e, double *cone_ms) {
    return jf_guard([&]() -> int {
    DeviceGuard bind(e);
    if (!e || !cone_ms) return JF_ERR_ARG;
    return e->cn.tm.sum(e, cone_ms);
    });
}

}  // extern "C"
