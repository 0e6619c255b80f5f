// swc_io.cpp -- the host's SWC files (see advantra_host.h): the reader of the tool modes, --swc-info, and the two writers of the
// tracing run.
#include "host_internal.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <unordered_map>

namespace advantra {

bool load_swc(const std::string &path, SwcTree &out, std::string &err)
{
    std::ifstream f(path);
    if (!f) {
        err = path + ": cannot open the file";
        return false;
    }
    out = SwcTree();
    std::vector<long long> pid;
    std::unordered_map<long long, int32_t> index;
    std::string line;
    for (long long ln = 1; std::getline(f, line); ln++) {
        std::istringstream is(line);
        std::vector<std::string> t;
        for (std::string w; is >> w;) t.push_back(w);
        if (t.empty() || t[0][0] == '#') continue;
        auto bad = [&](const std::string &what) {
            err = path + ":" + std::to_string(ln) + ": " + what;
            return false;
        };
        if (t.size() < 7) return bad("not an SWC line `n type x y z r parent` (" + std::to_string(t.size()) + " fields)");
        double v[7];
        for (int k = 0; k < 7; k++) {
            char *end = nullptr;
            v[k] = strtod(t[(size_t)k].c_str(), &end);
            if (*end || !std::isfinite(v[k])) return bad("field " + std::to_string(k + 1) + " `" + t[(size_t)k] + "` is not a number");
        }
        if (v[0] != std::floor(v[0]) || v[6] != std::floor(v[6]) || std::fabs(v[0]) > 9e15 || std::fabs(v[6]) > 9e15) return bad("the node id and the parent id must be whole numbers");
        const long long id = (long long)v[0];
        if (!index.emplace(id, (int32_t)out.id.size()).second) return bad("duplicate node id " + std::to_string(id));
        out.id.push_back(id);
        out.type.push_back((int32_t)v[1]);
        for (int k = 2; k < 5; k++) out.xyz.push_back((float)v[k]);
        out.radius.push_back((float)v[5]);
        pid.push_back((long long)v[6]);
    }
    out.parent.resize(pid.size());
    for (size_t i = 0; i < pid.size(); i++) {
        const auto it = pid[i] < 0 ? index.end() : index.find(pid[i]);
        out.parent[i] = it == index.end() ? -1 : it->second;
    }
    return true;
}

bool read_swc(const std::string &path, SwcTree &out)
{
    std::string err;
    if (load_swc(path, out, err)) return true;
    fprintf(stderr, "%s\n", err.c_str());
    return false;
}

bool print_swc_info(const std::string &path)
{
    SwcTree t;
    if (!read_swc(path, t)) return false;
    long long roots = 0;
    double length = 0;
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (long long i = 0; i < t.n(); i++) {
        const float *p = &t.xyz[(size_t)(3 * i)];
        for (int k = 0; k < 3; k++) lo[k] = std::min(lo[k], p[k]), hi[k] = std::max(hi[k], p[k]);
        if (t.parent[(size_t)i] < 0) {
            roots++;
            continue;
        }
        const float *q = &t.xyz[(size_t)(3 * (long long)t.parent[(size_t)i])];
        const double dx = (double)q[0] - p[0], dy = (double)q[1] - p[1], dz = (double)q[2] - p[2];
        length += std::sqrt((dx * dx + dy * dy) + dz * dz);
    }
    printf("{\"nodes\": %lld, \"roots\": %lld, \"segments\": %lld, \"length\": %.17g, \"bbox\": ", t.n(), roots, t.n() - roots, length);
    if (t.n()) printf("[%.9g, %.9g, %.9g, %.9g, %.9g, %.9g]}\n", lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    else printf("null}\n");
    return true;
}

std::string f32_text(float v)
{
    char buf[40];
    for (int prec = 1; prec <= 9; prec++) {
        snprintf(buf, sizeof buf, "%.*g", prec, (double)v);
        if ((float)strtod(buf, nullptr) == v && !strchr(buf, 'e')) break;
    }
    return buf;
}

// the file both writers start: the name line, the comment block and the column line (nullptr: the file cannot be written)
static FILE *open_swc(const std::string &swcname, const std::string &name, const std::string &comment)
{
    FILE *f = fopen(swcname.c_str(), "w");
    if (!f) return nullptr;
    if (!name.empty()) fprintf(f, "#name %s\n", name.c_str());
    std::stringstream ss(comment);
    std::string ln;
    for (bool first = true; std::getline(ss, ln);) {
        if (ln.empty()) continue;
        fprintf(f, "%s%s\n", (first || ln[0] != '#') ? "#comment " : "", ln.c_str());
        first = false;
    }
    fprintf(f, "##n,type,x,y,z,radius,parent\n");
    return f;
}

bool save_nodelist(const std::vector<pnr_node> &nodes, const std::vector<int32_t> &links, const std::string &swcname, int type,
                   float sig2r, const std::string &name, const std::string &comment, const std::vector<float> *radius)
{
    // one line per (node, neighbour) pair, ids repeat; isolated nodes get parent -1; node 0 is the dummy
    std::vector<std::vector<int>> nbr(nodes.size());
    for (size_t k = 0; k + 1 < links.size(); k += 2) { // a.nbr.push_back(b); b.nbr.push_back(a)
        nbr[links[k]].push_back(links[k + 1]);
        nbr[links[k + 1]].push_back(links[k]);
    }
    FILE *f = open_swc(swcname, name, comment);
    if (!f) return false;
    for (size_t i = 1; i < nodes.size(); i++) {
        const pnr_node &nd = nodes[i];
        const int t = (type == -1) ? nd.type : type;
        const float r = (radius && i < radius->size() && (*radius)[i] >= 0.f) ? (*radius)[i] : sig2r * nd.sig;
        if (nbr[i].empty()) fprintf(f, "%zu %d %.3f %.3f %.3f %.3f %d\n", i, t, nd.x, nd.y, nd.z, r, -1);
        for (int par : nbr[i]) fprintf(f, "%zu %d %.3f %.3f %.3f %.3f %d\n", i, t, nd.x, nd.y, nd.z, r, par);
    }
    fclose(f);
    return true;
}

bool save_treelist(const std::vector<pnr_node> &tree, const std::vector<int32_t> &parent, const std::string &swcname, int type,
                   float sig2r, const std::string &name, const std::string &comment, const std::vector<float> *radius)
{
    FILE *f = open_swc(swcname, name, comment);
    if (!f) return false;
    for (size_t i = 1; i < tree.size(); i++) {
        const pnr_node &nd = tree[i];
        const float r = (radius && i < radius->size() && (*radius)[i] >= 0.f) ? (*radius)[i] : sig2r * nd.sig;
        fprintf(f, "%zu %d %.3f %.3f %.3f %.3f %d\n", i, (type == -1) ? nd.type : type, nd.x, nd.y, nd.z, r, parent[i]);
    }
    fclose(f);
    return true;
}

} // namespace advantra
