// jf_cloud.cpp -- HRTF sets on arbitrary directions (include/jefferson.h: jf_cloud), host side, no GPU:
// the spherical Delaunay triangulation of the measurement directions (= the convex hull of their unit vectors), the
// triangle records and seed cells the kernels walk, and the host twin of the kernels' rule (jf_cloud_rule.h, compiled for
// both sides).  Product code; built with -ffp-contract=off like jf_host.cpp.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <string>
#include <vector>

#include "../../include/jefferson.h"
#include "jf_host.h"

namespace jf {
namespace {

typedef long double real;  // plane equations and heights: 64-bit mantissa on x86, so that what decides "coplanar" is the
                           // rounding of the input (the directions themselves are double), not of the cross products

struct Vec {
    double x, y, z;
};

struct Face {
    int v[3];   // outward (counter-clockwise seen from outside)
    int nb[3];  // the face across the edge opposite v[i]
    real nx, ny, nz, off;  // unit normal, n . v[0]
    bool alive;
};

// A direction counts as above a face's plane when it is higher than this.  Directions at least 0.001 degrees apart on the
// unit sphere lie >= 1e-10 above the faces they see; directions that are coplanar on paper (two azimuths on two rings) come
// out within ~1e-14 of the plane.  Such a face is NOT seen: the new triangle lies flat beside it, a valid triangulation of
// the planar patch -- no jitter of the input.
constexpr real kVisible = 1e-13L;
constexpr double kMinTolDeg = 1e-3;

void set_plane(const std::vector<Vec> &p, Face &f) {
    const Vec &a = p[f.v[0]], &b = p[f.v[1]], &c = p[f.v[2]];
    const real ux = (real)b.x - a.x, uy = (real)b.y - a.y, uz = (real)b.z - a.z;
    const real vx = (real)c.x - a.x, vy = (real)c.y - a.y, vz = (real)c.z - a.z;
    real nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const real len = sqrtl(nx * nx + ny * ny + nz * nz);
    if (len > 0) nx /= len, ny /= len, nz /= len;
    f.nx = nx, f.ny = ny, f.nz = nz;
    f.off = nx * a.x + ny * a.y + nz * a.z;
}

inline real height(const Face &f, const Vec &q) { return f.nx * q.x + f.ny * q.y + f.nz * q.z - f.off; }

// index in g of the edge (from -> to) as g runs it; -1 if g has no such edge
int edge_index(const Face &g, int from, int to) {
    for (int j = 0; j < 3; j++)
        if (g.v[(j + 1) % 3] == from && g.v[(j + 2) % 3] == to) return j;
    return -1;
}

// The convex hull of p (points on the unit sphere, all of them vertices): incremental, every face scanned per point
// (O(n * faces)).  tri: 2n - 4 outward triangles.
int hull(const std::vector<Vec> &p, std::vector<int> *tri, std::string *err) {
    const int n = (int)p.size();
    auto dist2 = [&](int i, int j) {
        const double dx = p[i].x - p[j].x, dy = p[i].y - p[j].y, dz = p[i].z - p[j].z;
        return dx * dx + dy * dy + dz * dz;
    };
    // a first tetrahedron of four directions far from one plane
    int i0 = 0, i1 = 0, i2 = 0, i3 = 0;
    double best = -1;
    for (int i = 0; i < n; i++)
        if (dist2(i0, i) > best) best = dist2(i0, i), i1 = i;
    best = -1;
    const Vec e1 = {p[i1].x - p[i0].x, p[i1].y - p[i0].y, p[i1].z - p[i0].z};
    for (int i = 0; i < n; i++) {
        const Vec d = {p[i].x - p[i0].x, p[i].y - p[i0].y, p[i].z - p[i0].z};
        const double cx = e1.y * d.z - e1.z * d.y, cy = e1.z * d.x - e1.x * d.z, cz = e1.x * d.y - e1.y * d.x;
        const double a2 = cx * cx + cy * cy + cz * cz;
        if (a2 > best) best = a2, i2 = i;
    }
    Face base{};
    base.v[0] = i0, base.v[1] = i1, base.v[2] = i2;
    set_plane(p, base);
    real besth = -1;
    for (int i = 0; i < n; i++) {
        const real h = fabsl(height(base, p[i]));
        if (h > besth) besth = h, i3 = i;
    }
    if (!(besth > 1e-9L)) {
        *err = "the directions lie in one plane: no triangulation of the sphere";
        return JF_ERR_ARG;
    }
    if (height(base, p[i3]) > 0) std::swap(i1, i2);  // (i0, i1, i2) now turns its back on i3
    std::vector<Face> F;
    F.reserve(2 * (size_t)n + 8);
    const int tv[4][3] = {{i0, i1, i2}, {i0, i3, i1}, {i1, i3, i2}, {i2, i3, i0}};
    for (int f = 0; f < 4; f++) {
        Face g{};
        for (int k = 0; k < 3; k++) g.v[k] = tv[f][k];
        g.alive = true;
        set_plane(p, g);
        F.push_back(g);
    }
    for (int f = 0; f < 4; f++)
        for (int j = 0; j < 3; j++) {
            const int from = F[f].v[(j + 1) % 3], to = F[f].v[(j + 2) % 3];
            int found = -1;
            for (int g = 0; g < 4; g++)
                if (g != f && edge_index(F[g], to, from) >= 0) found = g;
            if (found < 0) {
                *err = "triangulation failed (first tetrahedron)";
                return JF_ERR_ARG;
            }
            F[f].nb[j] = found;
        }
    std::vector<char> in_hull((size_t)n, 0);
    in_hull[i0] = in_hull[i1] = in_hull[i2] = in_hull[i3] = 1;
    std::vector<int> free_slots, visible, stack, start_at((size_t)n, -1), end_at((size_t)n, -1), fresh;
    std::vector<char> seen;
    struct Horizon {
        int u, v, outside;
    };
    std::vector<Horizon> horizon;
    for (int q = 0; q < n; q++) {
        if (in_hull[q]) continue;
        int top = -1;
        real toph = kVisible;
        for (int f = 0; f < (int)F.size(); f++) {
            if (!F[f].alive) continue;
            const real h = height(F[f], p[q]);
            if (h > toph) toph = h, top = f;
        }
        if (top < 0) {
            *err = "triangulation failed: direction " + std::to_string(q) + " does not lie outside the hull of the others";
            return JF_ERR_ARG;
        }
        // the faces the direction sees, from the one it is highest above through the neighbours
        seen.assign(F.size(), 0);
        visible.clear();
        stack.assign(1, top);
        seen[top] = 1;
        while (!stack.empty()) {
            const int f = stack.back();
            stack.pop_back();
            visible.push_back(f);
            for (int j = 0; j < 3; j++) {
                const int g = F[f].nb[j];
                if (!seen[g] && height(F[g], p[q]) > kVisible) {
                    seen[g] = 1;
                    stack.push_back(g);
                }
            }
        }
        horizon.clear();
        for (const int f : visible)
            for (int j = 0; j < 3; j++) {
                const int g = F[f].nb[j];
                if (!seen[g]) horizon.push_back({F[f].v[(j + 1) % 3], F[f].v[(j + 2) % 3], g});
            }
        // the horizon must be ONE closed chain: every vertex of it starts one edge and ends one
        bool ok = horizon.size() >= 3 && horizon.size() == visible.size() + 2;
        for (const Horizon &h : horizon) {
            if (start_at[h.u] != -1 || end_at[h.v] != -1) ok = false;
            start_at[h.u] = end_at[h.v] = 0;
        }
        for (const Horizon &h : horizon)
            if (start_at[h.v] == -1 || end_at[h.u] == -1) ok = false;
        if (!ok) {
            for (const Horizon &h : horizon) start_at[h.u] = end_at[h.v] = -1;
            *err = "triangulation failed: the faces direction " + std::to_string(q) + " sees do not form a disc";
            return JF_ERR_ARG;
        }
        for (const int f : visible) {
            F[f].alive = false;
            free_slots.push_back(f);
        }
        fresh.clear();
        for (const Horizon &h : horizon) {
            Face g{};
            g.v[0] = h.u, g.v[1] = h.v, g.v[2] = q;
            g.nb[2] = h.outside;
            g.alive = true;
            set_plane(p, g);
            int slot;
            if (!free_slots.empty()) {
                slot = free_slots.back();
                free_slots.pop_back();
                F[slot] = g;
            } else {
                slot = (int)F.size();
                F.push_back(g);
            }
            fresh.push_back(slot);
            start_at[h.u] = slot;
            end_at[h.v] = slot;
            const int j = edge_index(F[h.outside], h.v, h.u);
            if (j < 0) ok = false; else F[h.outside].nb[j] = slot;
        }
        for (const int s : fresh) {
            F[s].nb[0] = start_at[F[s].v[1]];  // across (v, q): the new face that starts at v
            F[s].nb[1] = end_at[F[s].v[0]];    // across (q, u): the new face that ends at u
        }
        for (const Horizon &h : horizon) start_at[h.u] = end_at[h.v] = -1;
        if (!ok) {
            *err = "triangulation failed (horizon of direction " + std::to_string(q) + ")";
            return JF_ERR_ARG;
        }
        in_hull[q] = 1;
    }
    tri->clear();
    std::vector<char> used((size_t)n, 0);
    for (const Face &f : F) {
        if (!f.alive) continue;
        // the hull must hold the origin strictly inside: a set that covers a hemisphere only has no answer on the far side
        if (!(f.off > 1e-6L)) {
            *err = "the directions cover a hemisphere only (the hull of their unit vectors does not hold the origin inside)";
            return JF_ERR_ARG;
        }
        for (int k = 0; k < 3; k++) {
            tri->push_back(f.v[k]);
            used[f.v[k]] = 1;
        }
    }
    if ((int)tri->size() != 3 * (2 * n - 4) || std::find(used.begin(), used.end(), 0) != used.end()) {
        *err = "triangulation failed: " + std::to_string(tri->size() / 3) + " triangles for " + std::to_string(n) + " directions";
        return JF_ERR_ARG;
    }
    return JF_OK;
}

// the triangle of greatest minimum lambda over ALL records, in the kernels' arithmetic (seed cells the walk cannot reach)
int brute_locate(const std::vector<CloudTri> &tri, double x, double y, double z) {
    int best = 0;
    float best_min = -3.0e38f;
    for (int t = 0; t < (int)tri.size(); t++) {
        float l0, l1, l2;
        cloud_lambda(tri[t], x, y, z, &l0, &l1, &l2);
        const float mn = std::min(l0, std::min(l1, l2));
        if (mn > best_min) best_min = mn, best = t;
    }
    return best;
}

}  // namespace

int cloud_build(size_t n_in, const float *azi, const float *ele, float tol_deg, jf_cloud *out, std::string *err) {
    if (!azi || !ele || !out) {
        *err = "null argument";
        return JF_ERR_ARG;
    }
    if (n_in < 4) {
        *err = "a cloud needs at least 4 directions";
        return JF_ERR_ARG;
    }
    if (n_in > (size_t)JF_CLOUD_MAX_DIRECTIONS) {
        *err = "more than " + std::to_string(JF_CLOUD_MAX_DIRECTIONS) + " directions";
        return JF_ERR_ARG;
    }
    if (!(tol_deg >= 0.0f) || !(tol_deg <= 90.0f)) {
        *err = "tol_deg must lie in [0, 90]";
        return JF_ERR_ARG;
    }
    const int n = (int)n_in;
    std::vector<Vec> p((size_t)n);
    for (int i = 0; i < n; i++) {
        if (!(fabsf(azi[i]) < 1.0e6f) || !(ele[i] >= -90.0f && ele[i] <= 90.0f)) {
            *err = "direction " + std::to_string(i) + ": non-finite value or elevation outside [-90, 90]";
            return JF_ERR_ARG;
        }
        const double a = (double)azi[i] * (M_PI / 180.0), e = (double)ele[i] * (M_PI / 180.0);
        p[i] = {cos(e) * sin(a), cos(e) * cos(a), sin(e)};  // jf_cloud_rule.h: x right, y front, z up
    }
    {
        const double tol = std::max((double)tol_deg, kMinTolDeg) * (M_PI / 180.0);
        const double chord2 = 4.0 * sin(tol / 2) * sin(tol / 2);
        // sorted by z: only directions within the chord in z are compared
        std::vector<int> order((size_t)n);
        for (int i = 0; i < n; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return p[a].z < p[b].z || (p[a].z == p[b].z && a < b); });
        const double chord = sqrt(chord2);
        for (int i = 0; i < n; i++)
            for (int j = i + 1; j < n && p[order[j]].z - p[order[i]].z < chord; j++) {
                const Vec &u = p[order[i]], &v = p[order[j]];
                const double d2 = (u.x - v.x) * (u.x - v.x) + (u.y - v.y) * (u.y - v.y) + (u.z - v.z) * (u.z - v.z);
                if (d2 < chord2) {
                    *err = "directions " + std::to_string(std::min(order[i], order[j])) + " and " +
                           std::to_string(std::max(order[i], order[j])) + " are closer than tol_deg";
                    return JF_ERR_ARG;
                }
            }
    }
    std::vector<int> tri;
    const int rc = hull(p, &tri, err);
    if (rc) return rc;
    const int nt = (int)tri.size() / 3;
    // every triangle from its lowest row on (the order stays outward), the triangles in ascending order of their rows
    std::vector<std::array<int, 3>> T((size_t)nt);
    for (int t = 0; t < nt; t++) {
        int *v = &tri[3 * (size_t)t];
        const int lo = v[0] < v[1] ? (v[0] < v[2] ? 0 : 2) : (v[1] < v[2] ? 1 : 2);
        T[t] = {v[lo], v[(lo + 1) % 3], v[(lo + 2) % 3]};
    }
    std::sort(T.begin(), T.end());
    // neighbours: the triangle that runs an edge the other way
    std::vector<std::pair<long long, int>> edges;  // (from * n + to, 3 t + index of the opposite vertex)
    edges.reserve(3 * (size_t)nt);
    for (int t = 0; t < nt; t++)
        for (int j = 0; j < 3; j++)
            edges.push_back({(long long)T[t][(j + 1) % 3] * n + T[t][(j + 2) % 3], 3 * t + j});
    std::sort(edges.begin(), edges.end());
    out->azi.assign(azi, azi + n);
    out->ele.assign(ele, ele + n);
    out->tri.assign((size_t)nt, CloudTri{});
    for (int t = 0; t < nt; t++) {
        CloudTri &r = out->tri[t];
        const Vec &a = p[T[t][0]], &b = p[T[t][1]], &c = p[T[t][2]];
        // [a b c]^-1: rows (b x c, c x a, a x b) / det
        const Vec bc = {b.y * c.z - b.z * c.y, b.z * c.x - b.x * c.z, b.x * c.y - b.y * c.x};
        const Vec ca = {c.y * a.z - c.z * a.y, c.z * a.x - c.x * a.z, c.x * a.y - c.y * a.x};
        const Vec ab = {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
        const double det = a.x * bc.x + a.y * bc.y + a.z * bc.z;
        if (!(det > 0)) {
            *err = "triangulation failed: a triangle of no volume";
            return JF_ERR_ARG;
        }
        const Vec rows3[3] = {bc, ca, ab};
        for (int i = 0; i < 3; i++) {
            r.m[3 * i + 0] = (float)(rows3[i].x / det);
            r.m[3 * i + 1] = (float)(rows3[i].y / det);
            r.m[3 * i + 2] = (float)(rows3[i].z / det);
            r.row[i] = T[t][i];
            const long long key = (long long)T[t][(i + 2) % 3] * n + T[t][(i + 1) % 3];  // the edge opposite i, reversed
            const auto it = std::lower_bound(edges.begin(), edges.end(), std::make_pair(key, -1));
            if (it == edges.end() || it->first != key || (it + 1 != edges.end() && (it + 1)->first == key)) {
                *err = "triangulation failed: an edge without exactly one neighbour";
                return JF_ERR_ARG;
            }
            r.nb[i] = it->second / 3;
        }
    }
    // seed cells over (elevation, azimuth): about two cells per triangle, so that the walk reads about two records
    int ne = (int)ceil(sqrt(2.0 * n));
    ne = std::max(8, std::min(256, ne));
    const int na = 2 * ne;
    out->seed.assign((size_t)ne * na, 0);
    CloudView &cv = out->view;
    cv.tri = out->tri.data();
    cv.seed = out->seed.data();
    cv.n_tri = nt;
    cv.n_ele = ne;
    cv.n_azi = na;
    cv.ele_scale = (float)ne / 180.0f;
    cv.azi_scale = (float)na / 360.0f;
    cv.pad = 0;
    for (int ie = 0; ie < ne; ie++)
        for (int ia = 0; ia < na; ia++) {
            const float e = -90.0f + ((float)ie + 0.5f) * (180.0f / (float)ne), a = ((float)ia + 0.5f) * (360.0f / (float)na);
            double x, y, z;
            cloud_direction(e, a, &x, &y, &z);
            int &cell = out->seed[(size_t)ie * na + ia];
            int t = -1;
            if (ia > 0 || ie > 0) {  // walk from the cell before (the row below for a row's first cell)
                const int start = ia > 0 ? out->seed[(size_t)ie * na + ia - 1] : out->seed[(size_t)(ie - 1) * na];
                // (the walk reads its start from the cell of (e, a): this one, or at the table's rim a neighbour that is set)
                const int ce = std::min(ne - 1, std::max(0, (int)((e + 90.0f) * cv.ele_scale)));
                const int ca = std::min(na - 1, std::max(0, (int)(a * cv.azi_scale)));
                int &read_cell = out->seed[(size_t)ce * na + ca];
                const int keep = read_cell;
                read_cell = start;
                CloudTri rec;
                float l0, l1, l2;
                int steps;
                t = cloud_locate(cv, e, a, x, y, z, &rec, &l0, &l1, &l2, &steps);
                read_cell = keep;
                if (std::min(l0, std::min(l1, l2)) < -kCloudSlack) t = -1;  // the cap or a cycle: search
            }
            cell = t >= 0 ? t : brute_locate(out->tri, x, y, z);
        }
    return JF_OK;
}

int cloud_interpolation(const jf_cloud *c, float ele, float azi, int rows[3], float w[3], int *steps) {
    int n_steps = 0;
    const int n = cloud_terms(c->view, ele, azi, &rows[0], &rows[1], &rows[2], &w[0], &w[1], &w[2], &n_steps);
    if (steps) *steps = n_steps;
    return n;
}

int cloud_pick_row(const jf_cloud *c, float ele, float azi) { return cloud_pick(c->view, ele, azi); }

}  // namespace jf
