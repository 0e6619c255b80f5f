// advantra_host.cpp -- see advantra_host.h.  Host orchestration only: every compute stage is a call
// through the C ABI into libpnr_hip.so.
#include "advantra_host.h"
#include "stack_io.h"
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <sstream>
#include <unordered_map>

namespace advantra {

static const int nrInputParams = 11; // Advantra_plugin.cpp:60

Settings &settings()
{
    static Settings s;
    return s;
}

void print_help()
{
    // wording of the reference's print_help (Advantra_plugin.cpp:125-148), shortened to the call contract
    printf("**** usage of Advantra tracing ****\n");
    printf("vaa3d -x Advantra -f advantra_func -i <inimg_file> -p <neuritesigmas> <somaradius> <tolerance> <znccth> <kappa> "
           "<step> <ni> <np> <zdist> <nodepervol> <vol>\n");
    printf("inimg_file     The input image (8- or 16-bit multi-page TIFF; 16-bit stacks are windowed to 8 bits)\n");
    printf("neuritesigmas  Comma delimited list of gaussian cross-section sigmas, e.g. 2,4,6\n");
    printf("somaradius     Soma radius (0: no soma)\n");
    printf("tolerance      Seed extraction (find maxima) tolerance\n");
    printf("znccth         Correlation threshold [0,1]\n");
    printf("kappa          Von Mises kappa [0,5]\n");
    printf("step           Prediction step\n");
    printf("ni             Number of iterations\n");
    printf("np             Number of particles\n");
    printf("zdist          Distance between layers in pixels\n");
    printf("nodepervol     Node density limit (2,20]\n");
    printf("vol            Volume pattern: 1,5,9,11,19,27\n");
    printf("outswc_file    <inimg_file>_Advantra.swc\n");
}

void print_flags()
{
    printf("\nadvantra_cli [flags] -f advantra_func -i <inimg_file> -p <the 11 parameters>   (flags go before -p)\n");
    printf("-v | --timing | --save-midres | --single-tree | --rng-seed N | -g DEVICE | -d w,h,l (.raw) | --info\n");
    printf("--ranks N [--share-gpu] [--exchange shm|rccl]   one stack on N GPUs of this host\n");
    printf("--swc-info FILE.swc       one JSON line about an SWC file: nodes, roots, segments, total length, bounding box (no GPU)\n");
    printf("--distance A.swc B.swc    the tree distance of two SWC files on the GPU (SD, SSD, %%SSD per direction and combined) as one JSON line\n");
    printf("  --distance-step S         resampling step of both trees (default 1; 0: the nodes only)\n");
    printf("  --distance-threshold T    a point counts as far away from T on (default 2)\n");
    printf("  --zscale Z                z is multiplied by Z first (default 1; the stack's zdist gives distances in xy voxels)\n");
    printf("  --per-node PREFIX         also write PREFIX_ab.csv / PREFIX_ba.csv: `id,d` of every sample point of A / of B\n");
    printf("--join GAP                join the traced forest into one tree on the GPU: fragments whose closest nodes lie within GAP xy voxels\n");
    printf("                          (0: any distance) are bridged, the tree is re-rooted and written with every parent before its children\n");
    printf("  --join-root soma|ID       the root: the first soma node if there is one (default), or the node with this id in the file without --join\n");
    printf("  --join-keep-largest       write only the largest component (the root's, if a root is given)\n");
    printf("--join-swc IN.swc OUT.swc the same on an SWC file ([--join GAP] [--zscale Z] [--join-root ID] [--join-keep-largest]); one JSON line\n");
    printf("--render-swc IN.swc       render an SWC file into the stack given with -i (the same volume setup as tracing) on the GPU; one JSON line with\n");
    printf("                          the coverage counts: how much of the foreground the tree covers, how much of the tree lies on signal\n");
    printf("  --mask OUT                write the mask (255 under the tree) as a multi-page 8-bit TIFF, or bare bytes for a .raw name\n");
    printf("  --residual OUT            write the stack with the tree's voxels set to 0: the signal the trace does not explain\n");
    printf("  --per-node FILE.csv       `id,vox,fg,sum` per node: its voxels, the foreground among them, their summed intensity\n");
    printf("  --zscale Z | --radius-scale S | --radius-add A   z and the radii as rendered: z * Z, max(radius * S + A, 0)\n");
    printf("  --coverage-threshold T    foreground from T on, 0..255 (default -1: the stack's mean)\n");
    printf("                          without -i: -d w,h,l gives the grid and only --mask is allowed\n");
    printf("--mask OUT | --residual OUT | --coverage   while tracing: the final tree rendered on the traced stack (zscale = zdist); the comment block\n");
    printf("                          gains #coverage=thr:T,covered:..,on_signal:..,intensity:..,tree_voxels:N\n");
    printf("--channel C | --raw-type u8|u16 | --window LO,HI | --saturate LO,HI   the input; 16-bit stacks are windowed to 8 bits\n");
    printf("--median 2d|3d            pre-filter: 3 x 3 median in every slice, or 3 x 3 x 3 (on the GPU, before tracing; default: off)\n");
    printf("--subtract-background R   pre-filter: top-hat with a flat box of half-width R in xy and R / zdist in z, 1..%d (after the median)\n", PNR_TOPHAT_MAX_R);
    printf("--despeckle MIN[,THR[,CONN]]  pre-filter: foreground components (voxels >= THR, default -1: the stack's mean; CONN 6 or 26, default 26) of\n");
    printf("                          fewer than MIN voxels are set to 0 on the GPU (after the median and the top-hat, before tracing)\n");
    printf("--components -i stack     the connected components of the stack's foreground on the GPU (the same volume setup as tracing) as one JSON\n");
    printf("                          line: n_vox, n_fg, n_comp, n_small, vox_small, largest, thr_used; on a --residual file: what the trace missed\n");
    printf("  --threshold T             foreground from T on, 0..255 (default -1: the stack's mean)\n");
    printf("  --connectivity 6|26       face neighbours only, or faces, edges and corners (default 26)\n");
    printf("  --min-size M              components of fewer than M voxels are not counted, numbered or listed (default 1)\n");
    printf("  --labels OUT.raw          write the label volume: little-endian int32, 0 = background, 1.. by first voxel in raster order\n");
    printf("  --per-component FILE.csv  `id,size,sum,cx,cy,cz,x0,y0,z0,x1,y1,z1,vmax` per component\n");
    printf("--edt -i stack            the exact Euclidean distance transform of the stack's foreground on the GPU (the same volume setup as tracing):\n");
    printf("                          every voxel's distance d to the nearest background voxel, in xy voxels; one JSON line: n_vox, n_fg, n_capped,\n");
    printf("                          thr_used, rmax, zdist, d_max, max_at (the thickest point: where a soma is, and how large somaradius has to be)\n");
    printf("  --threshold T             foreground from T on, 0..255 (default -1: the stack's mean)\n");
    printf("  --edt-max R               distances are capped at R xy voxels, 1..%d (default 64)\n", PNR_EDT_MAX_R);
    printf("  --zscale Z                z counts Z-fold, 1 or more (default 1)\n");
    printf("  --edt-out OUT.raw         write d of every voxel: little-endian float32\n");
    printf("  --at tree.swc --per-node FILE.csv   `id,d` per node of the SWC file: its sub-voxel radius (-1: a position that is not finite)\n");
    printf("--geodesic -i stack --from tree.swc   the gray-weighted geodesic distance of every voxel to the tree on the GPU (the same volume setup as\n");
    printf("                          tracing): the cheapest 26-connected path, a step costs its length times the darkness 256 - v of its two voxels;\n");
    printf("                          one JSON line: n_vox, n_pass, n_reached, n_src, n_src_dropped, thr_used, dmax, zdist, d_max, len_max, max_at, rounds\n");
    printf("  --threshold T             voxels below T are impassable, 0..255, -1: the stack's mean (default 0: every voxel is passable)\n");
    printf("  --geo-max D               no path that costs more than D is kept, 1..2147483647 (default: no limit; 64 is one xy voxel at cost 1)\n");
    printf("  --zscale Z                z counts Z-fold, 1 or more (default 1)\n");
    printf("  --to other.swc --per-node FILE.csv   `id,d,label` per node of the SWC file: its cost and the id of the tree node it attaches to\n");
    printf("  --paths OUT.swc           with --to: every complete path as a chain of SWC nodes that ends on the tree (paths of more than\n");
    printf("                            min(%d, 2^26 / nodes) voxels are left out and counted on stderr)\n", PNR_GEO_MAX_PATH);
    printf("  --geo-out PREFIX          write PREFIX_d.raw (little-endian uint32, 4294967295: unreached) and PREFIX_label.raw (int32, -1: unreached)\n");
    printf("--measure-radius          SWC radii measured from the image at the final nodes (default: SIG2RADIUS * the winning scale)\n");
    printf("--radius-rel PCT          relative mode (default, 50): background below PCT %% of the node's brightest centre voxel, 1..100\n");
    printf("--radius-threshold T      absolute mode: background below T, 0..255; -1: below the stack's mean\n");
    printf("--radius-max K            largest radius looked for, in xy voxels, 1..%d (default 32)\n", PNR_RADIUS_MAX);
    printf("--radius-bg PERMILLE      background voxels a ball may hold, per thousand, 0..999 (default 1)\n");
}

// ---- baseline TIFF reader: 8- or 16-bit unsigned samples in either byte order, uncompressed strips, any number of pages; several
// samples per pixel (chunky or planar) or ImageJ hyperstack channels, of which one is kept ----
namespace {
struct Reader {
    std::vector<unsigned char> buf;
    bool be = false;
    uint16_t u16(size_t o) const { return be ? (uint16_t)(buf[o] << 8 | buf[o + 1]) : (uint16_t)(buf[o] | buf[o + 1] << 8); }
    uint32_t u32(size_t o) const
    {
        return be ? ((uint32_t)buf[o] << 24 | (uint32_t)buf[o + 1] << 16 | (uint32_t)buf[o + 2] << 8 | buf[o + 3])
                  : ((uint32_t)buf[o + 3] << 24 | (uint32_t)buf[o + 2] << 16 | (uint32_t)buf[o + 1] << 8 | buf[o]);
    }
    std::vector<uint32_t> values(uint16_t type, uint32_t count, size_t field) const
    {
        const size_t sz = (type == 3) ? 2 : (type == 4 ? 4 : 1);
        size_t off = (sz * count <= 4) ? field : u32(field);
        if (off > buf.size() || (size_t)count > (buf.size() - off) / sz) return {}; // a count the file cannot hold: nothing is allocated for it
        std::vector<uint32_t> v(count);
        for (uint32_t i = 0; i < count; i++) {
            if (off + sz > buf.size()) return {};
            v[i] = (type == 3) ? u16(off) : (type == 4 ? u32(off) : buf[off]);
            off += sz;
        }
        return v;
    }
};

struct Page {
    uint32_t w = 0, h = 0, bps = 1, comp = 1, spp = 1, planar = 1, fmt = 1;
    bool mixed = false; // BitsPerSample / SampleFormat differ between the samples of a pixel
    std::vector<uint32_t> soff, scnt;
};

// the whole file in one read
bool read_file(const std::string &path, std::vector<unsigned char> &buf, std::string &err)
{
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) { err = "cannot open " + path; return false; }
    struct stat sb;
    if (fstat(fd, &sb) != 0) { close(fd); err = "cannot open " + path; return false; }
    buf.resize((size_t)sb.st_size);
    size_t got = 0;
    while (got < buf.size()) {
        const ssize_t n = read(fd, buf.data() + got, buf.size() - got);
        if (n <= 0) break;
        got += (size_t)n;
    }
    close(fd);
    if (got != buf.size()) { err = "cannot read " + path; return false; }
    return true;
}

// "key=value" of an ImageJ description (0 when absent)
long long imagej_value(const std::string &desc, const std::string &key)
{
    size_t at = 0;
    while ((at = desc.find(key + "=", at)) != std::string::npos) {
        if (at == 0 || desc[at - 1] == '\n') return atoll(desc.c_str() + at + key.size() + 1);
        at++;
    }
    return 0;
}
} // namespace

static bool load_tiff(const std::string &path, int channel, Stack &out, std::string &err)
{
    Reader r;
    if (!read_file(path, r.buf, err)) return false;
    if (r.buf.size() < 8) { err = "not a TIFF"; return false; }
    if (r.buf[0] == 'M' && r.buf[1] == 'M') r.be = true;
    else if (!(r.buf[0] == 'I' && r.buf[1] == 'I')) { err = "not a TIFF"; return false; }
    if (r.u16(2) != 42) { err = "not a baseline TIFF (BigTIFF is not supported)"; return false; }
    size_t ifd = r.u32(4);
    out.data.clear();
    out.data16.clear();
    out.w = out.h = out.l = 0;
    std::vector<Page> pages;
    std::string desc; // ImageDescription of the first page
    std::vector<size_t> seen; // IFD offsets visited: a chain that revisits one would never end
    while (ifd != 0) {
        if (ifd + 2 > r.buf.size()) { err = "truncated TIFF"; return false; }
        if (std::find(seen.begin(), seen.end(), ifd) != seen.end()) { err = "TIFF directory chain loops"; return false; }
        seen.push_back(ifd);
        if (seen.size() > (1u << 20)) { err = "TIFF with more than 2^20 pages"; return false; }
        const uint16_t n = r.u16(ifd);
        Page pg;
        for (uint16_t e = 0; e < n; e++) {
            const size_t o = ifd + 2 + 12 * (size_t)e;
            if (o + 12 > r.buf.size()) { err = "truncated TIFF"; return false; }
            const uint16_t tag = r.u16(o), type = r.u16(o + 2);
            const uint32_t cnt = r.u32(o + 4);
            if (tag == 270 && !pages.empty()) continue; // only the first page's description is read
            const std::vector<uint32_t> v = r.values(type, cnt, o + 8);
            if (v.empty()) continue;
            const bool same = std::all_of(v.begin(), v.end(), [&](uint32_t x) { return x == v[0]; });
            switch (tag) {
            case 256: pg.w = v[0]; break;
            case 257: pg.h = v[0]; break;
            case 258: pg.bps = v[0]; pg.mixed |= !same; break;
            case 259: pg.comp = v[0]; break;
            case 270: if (type == 2) desc.assign(v.begin(), std::find(v.begin(), v.end(), 0u)); break;
            case 273: pg.soff = v; break;
            case 277: pg.spp = v[0]; break;
            case 279: pg.scnt = v; break;
            case 284: pg.planar = v[0]; break;
            case 339: pg.fmt = v[0]; pg.mixed |= !same; break;
            }
        }
        if (pg.fmt != 1) { err = "only unsigned integer samples are supported (SampleFormat = " + std::to_string(pg.fmt) + ")"; return false; }
        if (pg.bps != 8 && pg.bps != 16) { err = "only 8- and 16-bit samples are supported (BitsPerSample = " + std::to_string(pg.bps) + ")"; return false; }
        if (pg.mixed) { err = "samples of different depth or format in one pixel"; return false; }
        if (pg.comp != 1) { err = "compressed TIFF is not supported"; return false; }
        if (pg.spp < 1) { err = "SamplesPerPixel = 0"; return false; }
        // uncompressed: the page's samples must be in the file
        if (pg.w == 0 || pg.h == 0 || (uint64_t)pg.w * pg.h * pg.spp * (pg.bps / 8) > r.buf.size()) { err = "TIFF page larger than the file"; return false; }
        if (!pages.empty() && (pg.w != pages[0].w || pg.h != pages[0].h)) { err = "pages of different size"; return false; }
        if (!pages.empty() && (pg.bps != pages[0].bps || pg.spp != pages[0].spp)) { err = "pages of different sample layout"; return false; }
        pages.push_back(std::move(pg));
        const size_t nx = ifd + 2 + 12 * (size_t)n;
        if (nx + 4 > r.buf.size()) break;
        ifd = r.u32(nx);
    }
    if (pages.empty()) { err = "TIFF without pages"; return false; }
    // ImageJ hyperstack: the pages run channel-fastest (c0 z0, c1 z0, ..., c0 z1, ...)
    long long nchan_ij = 1;
    if (desc.rfind("ImageJ=", 0) == 0) {
        const long long frames = imagej_value(desc, "frames");
        if (frames > 1) { err = "time series are not supported (ImageJ frames=" + std::to_string(frames) + ")"; return false; }
        nchan_ij = std::max(1LL, imagej_value(desc, "channels"));
        if (nchan_ij > 1 && pages[0].spp > 1) { err = "ImageJ hyperstack with several samples per pixel is not supported"; return false; }
        if ((long long)pages.size() % nchan_ij != 0) { err = "ImageJ hyperstack: " + std::to_string(pages.size()) + " pages are not a multiple of channels=" + std::to_string(nchan_ij); return false; }
    }
    const int spp = (int)pages[0].spp, B = (int)pages[0].bps / 8;
    out.bits = 8 * B;
    out.channels = nchan_ij > 1 ? (int)nchan_ij : spp;
    if (channel < 0 || channel >= out.channels) { err = "Invalid channel number."; return false; } // Advantra_plugin.cpp:2245-2249
    out.channel = channel;
    const uint32_t w = pages[0].w, h = pages[0].h;
    const size_t npix = (size_t)w * h;
    const size_t nplanes = pages.size() / (size_t)nchan_ij;
    // every sample kept is in the file: reserving for them is bounded by the file's size
    const size_t reserve = std::min(nplanes * npix, r.buf.size() / (size_t)B);
    if (B == 1) out.data.reserve(reserve);
    else out.data16.reserve(reserve);
    for (size_t z = 0; z < nplanes; z++) {
        const Page &pg = pages[nchan_ij > 1 ? z * (size_t)nchan_ij + (size_t)channel : z];
        // the page's stream of samples: interleaved (chunky, stride spp) or, planar, the strips of the kept channel's plane alone
        int stride = nchan_ij > 1 ? 1 : spp, sel = nchan_ij > 1 ? 0 : channel;
        size_t s0 = 0, s1 = pg.soff.size();
        if (pg.planar == 2 && spp > 1) {
            if (pg.soff.size() % (size_t)spp != 0) { err = "planar TIFF: StripOffsets is not a multiple of SamplesPerPixel"; return false; }
            const size_t sp = pg.soff.size() / (size_t)spp;
            s0 = sp * (size_t)channel;
            s1 = s0 + sp;
            stride = 1;
            sel = 0;
        }
        const size_t need = npix * (size_t)stride * (size_t)B; // bytes of the stream
        const size_t base = z * npix;
        if (B == 1) out.data.resize(base + npix);
        else out.data16.resize(base + npix);
        size_t pos = 0;
        for (size_t s = s0; s < s1 && pos < need; s++) {
            size_t c = (s < pg.scnt.size()) ? pg.scnt[s] : need - pos; // (StripByteCounts runs parallel to StripOffsets)
            c = std::min(c, need - pos);
            if ((size_t)pg.soff[s] + c > r.buf.size()) { err = "truncated TIFF strip"; return false; }
            if (c % (size_t)B) { err = "TIFF strip ends inside a sample"; return false; }
            const unsigned char *src = r.buf.data() + pg.soff[s];
            if (stride == 1 && B == 1) std::memcpy(out.data.data() + base + pos, src, c);
            else if (stride == 1 && !r.be) std::memcpy(out.data16.data() + base + pos / 2, src, c); // (little-endian host)
            else { // the kept channel's samples of this strip, de-interleaved and in the host's byte order
                const size_t q0 = pos / (size_t)B, q1 = (pos + c) / (size_t)B;
                for (size_t k = q0 + ((size_t)sel + (size_t)stride - q0 % (size_t)stride) % (size_t)stride; k < q1; k += (size_t)stride) {
                    const size_t o = pg.soff[s] + (k * (size_t)B - pos);
                    if (B == 1) out.data[base + k / (size_t)stride] = r.buf[o];
                    else out.data16[base + k / (size_t)stride] = r.u16(o);
                }
            }
            pos += c;
        }
        if (pos != need) { err = "TIFF page shorter than width*height"; return false; }
    }
    out.w = w; out.h = h; out.l = (long long)nplanes;
    return out.l > 0;
}

bool load_stack(const std::string &path, const std::string &raw_dims, Stack &out, std::string &err, int channel, bool raw_u16)
{
    const bool raw = path.size() > 4 && path.substr(path.size() - 4) == ".raw";
    if (!raw) return load_tiff(path, channel, out, err);
    long long w = 0, h = 0, l = 0;
    if (sscanf(raw_dims.c_str(), "%lld,%lld,%lld", &w, &h, &l) != 3 || w <= 0 || h <= 0 || l <= 0) {
        err = "raw stacks need -d w,h,l";
        return false;
    }
    if (channel != 0) { err = "Invalid channel number."; return false; } // a raw stack has one channel
    const long long B = raw_u16 ? 2 : 1, bytes = w * h * l * B;
    out.bits = (int)(8 * B);
    out.channels = 1;
    out.channel = 0;
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) { err = "cannot open " + path; return false; }
    struct stat sb;
    if (fstat(fd, &sb) != 0 || (long long)sb.st_size < bytes) { close(fd); err = raw_u16 ? "raw file shorter than 2*w*h*l" : "raw file shorter than w*h*l"; return false; }
    void *m = mmap(nullptr, (size_t)bytes, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) { // (a file system that cannot map: read it)
        std::ifstream f(path, std::ios::binary);
        if (!f) { err = "cannot open " + path; return false; }
        char *dst = nullptr;
        if (raw_u16) { out.data16.resize((size_t)(w * h * l)); dst = (char *)out.data16.data(); } // (u16 little-endian = the host's order)
        else { out.data.resize((size_t)(w * h * l)); dst = (char *)out.data.data(); }
        f.read(dst, (std::streamsize)bytes);
        if ((long long)f.gcount() != bytes) { err = "raw file shorter than w*h*l"; return false; }
    } else {
        out.view = (const unsigned char *)m;
        out.map_len = (size_t)bytes;
        (void)madvise(m, out.map_len, MADV_SEQUENTIAL);
    }
    out.w = w; out.h = h; out.l = l;
    return true;
}

bool print_info(const std::string &path, const std::string &raw_dims, int channel, bool raw_u16)
{
    Stack st;
    std::string err;
    if (!load_stack(path, raw_dims, st, err, channel, raw_u16)) {
        fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
    const size_t n = (size_t)(st.w * st.h * st.l);
    unsigned mn = 0xffffffffu, mx = 0;
    unsigned long long sum = 0;
    auto scan = [&](const auto *p) {
        for (size_t i = 0; i < n; i++) {
            const unsigned v = p[i];
            mn = std::min(mn, v);
            mx = std::max(mx, v);
            sum += v;
        }
    };
    if (st.bits == 16) scan(st.samples16());
    else scan(st.bytes());
    printf("{\"w\": %lld, \"h\": %lld, \"l\": %lld, \"bits\": %d, \"channels\": %d, \"channel\": %d, \"min\": %u, \"max\": %u, \"sum\": %llu}\n", st.w, st.h,
           st.l, st.bits, st.channels, channel + 1, mn, mx, sum);
    return true;
}

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

bool print_swc_info(const std::string &path)
{
    SwcTree t;
    std::string err;
    if (!load_swc(path, t, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
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

bool print_tree_distance(const std::string &a, const std::string &b, const pnr_distance_opts &opts, int device, const std::string &per_node)
{
    SwcTree A, B;
    std::string err;
    if (!load_swc(a, A, err) || !load_swc(b, B, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
    for (const auto &side : {std::make_pair(&a, &A), std::make_pair(&b, &B)})
        if (side.second->n() == 0) {
            fprintf(stderr, "%s: no nodes\n", side.first->c_str());
            return false;
        }
    auto lib_fail = [](const char *what) {
        fprintf(stderr, "%s: %s\n", what, pnr_last_error());
        return false;
    };
    // the sample points of either side first: the sizes of the per-point arrays (and an empty or malformed tree before any GPU work)
    int64_t na = 0, nb = 0;
    if (pnr_tree_sample(A.xyz.data(), A.parent.data(), A.n(), opts.zscale, opts.step, nullptr, nullptr, 0, &na) != PNR_OK) return lib_fail(a.c_str());
    if (pnr_tree_sample(B.xyz.data(), B.parent.data(), B.n(), opts.zscale, opts.step, nullptr, nullptr, 0, &nb) != PNR_OK) return lib_fail(b.c_str());
    pnr_params p;
    pnr_default_params(&p);
    pnr_ctx *ctx = nullptr;
    if (pnr_create(&p, device, &ctx) != PNR_OK) return lib_fail("pnr_create");
    std::vector<float> da((size_t)na), db((size_t)nb);
    std::vector<int32_t> oa((size_t)na), ob((size_t)nb);
    pnr_distance_result r;
    const int rc = pnr_tree_distance(ctx, A.xyz.data(), A.parent.data(), A.n(), B.xyz.data(), B.parent.data(), B.n(), &opts, &r, da.data(), oa.data(), na,
                                     db.data(), ob.data(), nb);
    pnr_destroy(ctx);
    if (rc != PNR_OK) return lib_fail("pnr_tree_distance");
    if (!per_node.empty()) {
        const struct { const char *tag; const SwcTree &t; const std::vector<float> &d; const std::vector<int32_t> &o; } side[2] = {{"_ab.csv", A, da, oa}, {"_ba.csv", B, db, ob}};
        for (const auto &s : side) {
            const std::string name = per_node + s.tag;
            FILE *f = fopen(name.c_str(), "w");
            if (!f) {
                fprintf(stderr, "%s: cannot write the file\n", name.c_str());
                return false;
            }
            fprintf(f, "id,d\n");
            for (size_t k = 0; k < s.d.size(); k++) fprintf(f, "%lld,%.9g\n", s.t.id[(size_t)s.o[k]], (double)s.d[k]);
            if (fclose(f) != 0) {
                fprintf(stderr, "%s: write failed\n", name.c_str());
                return false;
            }
        }
    }
    auto dir = [](const char *k, const pnr_distance_dir &d) {
        printf("\"%s\": {\"n\": %lld, \"n_big\": %lld, \"mean\": %.17g, \"ssd\": %.17g, \"pct\": %.17g, \"max\": %.17g}, ", k, (long long)d.n, (long long)d.n_big, d.mean,
               d.ssd, d.pct, d.max);
    };
    printf("{\"zscale\": %.9g, \"step\": %.9g, \"thr\": %.9g, \"nodes_a\": %lld, \"nodes_b\": %lld, ", (double)opts.zscale, (double)opts.step, (double)opts.thr, A.n(), B.n());
    dir("ab", r.ab);
    dir("ba", r.ba);
    printf("\"sd\": %.17g, \"ssd\": %.17g, \"pct\": %.17g, \"hausdorff\": %.17g}\n", r.sd, r.ssd, r.pct, r.hausdorff);
    return true;
}

// the shortest decimal text without an exponent (nine digits at the most) that reads back as the same f32
static std::string f32_text(float v)
{
    char buf[40];
    for (int prec = 1; prec <= 9; prec++) {
        snprintf(buf, sizeof buf, "%.*g", prec, (double)v);
        if ((float)strtod(buf, nullptr) == v && !strchr(buf, 'e')) break;
    }
    return buf;
}

bool join_swc_file(const std::string &in, const std::string &out, float gap, float zscale, long long root_id, bool keep_largest, int device)
{
    SwcTree T;
    std::string err;
    if (!load_swc(in, T, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
    const int64_t n = T.n();
    if (n == 0) {
        fprintf(stderr, "%s: no nodes\n", in.c_str());
        return false;
    }
    int64_t root = -1;
    if (root_id > 0) {
        const auto it = std::find(T.id.begin(), T.id.end(), root_id);
        if (it == T.id.end()) {
            fprintf(stderr, "--join-root %lld: %s has no node with this id\n", root_id, in.c_str());
            return false;
        }
        root = it - T.id.begin();
    }
    auto lib_fail = [](const char *what) {
        fprintf(stderr, "%s: %s\n", what, pnr_last_error());
        return false;
    };
    pnr_params p;
    pnr_default_params(&p);
    pnr_ctx *ctx = nullptr;
    if (pnr_create(&p, device, &ctx) != PNR_OK) return lib_fail("pnr_create");
    const pnr_join_opts jo = {zscale, gap, (int32_t)root};
    std::vector<int32_t> par_out((size_t)n), order((size_t)n), comp((size_t)n);
    std::vector<pnr_bridge> bridges((size_t)n);
    int64_t nb = 0, t_in = 0, t_out = 0, rounds = 0;
    const int rc = pnr_join_trees(ctx, T.xyz.data(), T.parent.data(), n, &jo, par_out.data(), order.data(), comp.data(), bridges.data(), n, &nb, &t_in, &t_out);
    pnr_get_option(ctx, "join_rounds", &rounds);
    pnr_destroy(ctx);
    if (rc != PNR_OK) return lib_fail("pnr_join_trees");
    FILE *f = fopen(out.c_str(), "w");
    if (!f) {
        fprintf(stderr, "%s: cannot write the file\n", out.c_str());
        return false;
    }
    fprintf(f, "#join=gap:%s,bridges:%lld,trees:%lld->%lld\n##n,type,x,y,z,radius,parent\n", f32_text(gap).c_str(), (long long)nb, (long long)t_in, (long long)t_out);
    std::vector<int64_t> pos((size_t)n, -1);
    int64_t written = 0;
    for (int64_t k = 0; k < n; k++) {
        const size_t v = (size_t)order[(size_t)k];
        if (keep_largest && comp[v] != 0) break;
        pos[v] = ++written;
        fprintf(f, "%lld %d %s %s %s %s %lld\n", (long long)written, T.type[v], f32_text(T.xyz[3 * v]).c_str(), f32_text(T.xyz[3 * v + 1]).c_str(),
                f32_text(T.xyz[3 * v + 2]).c_str(), f32_text(T.radius[v]).c_str(), par_out[v] < 0 ? -1LL : (long long)pos[(size_t)par_out[v]]);
    }
    if (fclose(f) != 0) {
        fprintf(stderr, "%s: write failed\n", out.c_str());
        return false;
    }
    printf("{\"nodes\": %lld, \"trees_in\": %lld, \"trees_out\": %lld, \"bridges\": %lld, \"longest_bridge\": %.9g, \"rounds\": %lld}\n", (long long)written,
           (long long)t_in, (long long)t_out, (long long)nb, nb ? (double)bridges[(size_t)nb - 1].d : 0.0, (long long)rounds);
    return true;
}

bool render_swc_file(const RenderJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, int device)
{
    SwcTree T;
    std::string err;
    if (!load_swc(job.swc, T, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
    auto lib_fail = [](const char *what) {
        fprintf(stderr, "%s: %s\n", what, pnr_last_error());
        return false;
    };
    auto write_stack = [&](const std::string &name, const std::vector<unsigned char> &vol, long long w, long long h, long long l) {
        std::string e;
        if (save_stack_u8(name, vol.data(), w, h, l, e)) return true;
        fprintf(stderr, "%s\n", e.c_str());
        return false;
    };
    const Settings &S = settings();
    const int64_t n = T.n();
    pnr_params p;
    pnr_default_params(&p);
    if (job.opts.zscale >= 1.f) p.zdist = job.opts.zscale; // (the z half-width of --subtract-background)
    int64_t items = 0;
    if (infiles.empty()) { // the mask alone, on the grid of -d
        long long w = 0, h = 0, l = 0;
        if (sscanf(raw_dims.c_str(), "%lld,%lld,%lld", &w, &h, &l) != 3 || w <= 0 || h <= 0 || l <= 0) {
            fprintf(stderr, "--render-swc without -i needs the grid: -d w,h,l\n");
            return false;
        }
        std::string e;
        if (job.mask.size() > 4 && job.mask.substr(job.mask.size() - 4) != ".raw" && tiff_u8_bytes(w, h, l) < 0 && !save_stack_u8(job.mask, nullptr, w, h, l, e)) {
            fprintf(stderr, "%s\n", e.c_str()); // (refused from the dimensions, before any GPU work)
            return false;
        }
        pnr_ctx *ctx = nullptr;
        if (pnr_create(&p, device, &ctx) != PNR_OK) return lib_fail("pnr_create");
        std::vector<unsigned char> mask((size_t)(w * h * l));
        const int rc = pnr_render_tree(ctx, T.xyz.data(), T.radius.data(), T.parent.data(), n, w, h, l, &job.opts, nullptr, mask.data());
        pnr_get_option(ctx, "render_items", &items);
        pnr_destroy(ctx);
        if (rc != PNR_OK) return lib_fail("pnr_render_tree");
        if (!write_stack(job.mask, mask, w, h, l)) return false;
        long long n_tree = 0;
        for (unsigned char v : mask) n_tree += v != 0;
        printf("{\"n_vox\": %lld, \"n_tree\": %lld, \"nodes\": %lld, \"items\": %lld}\n", w * h * l, n_tree, (long long)n, (long long)items);
        return true;
    }
    Stack st;
    if (!load_stack(infiles[0], raw_dims, st, err, S.channel - 1, S.raw_u16)) {
        fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
    if (S.windowed && st.bits != 16) {
        fprintf(stderr, "--window / --saturate need a 16-bit stack (8-bit input is never windowed)\n");
        return false;
    }
    pnr_ctx *ctx = nullptr;
    if (pnr_create(&p, device, &ctx) != PNR_OK) return lib_fail("pnr_create");
    // the volume as it would be traced: windowed to 8 bits, then pre-filtered
    bool ok = (st.bits == 16 ? pnr_set_volume_u16(ctx, st.samples16(), st.w, st.h, st.l, 1, 0, S.windowed ? &S.window : nullptr, nullptr, nullptr)
                             : pnr_set_volume(ctx, st.bytes(), st.w, st.h, st.l)) == PNR_OK;
    if (ok && (S.filter.median || S.filter.tophat_r)) ok = pnr_filter_volume(ctx, &S.filter) == PNR_OK;
    if (!ok) {
        lib_fail("volume");
        pnr_destroy(ctx);
        return false;
    }
    const size_t N = (size_t)(st.w * st.h * st.l);
    std::vector<unsigned char> mask(job.mask.empty() ? 0 : N), residual(job.residual.empty() ? 0 : N);
    std::vector<int64_t> vox, fg, sum;
    if (!job.per_node.empty()) vox.assign((size_t)n, 0), fg.assign((size_t)n, 0), sum.assign((size_t)n, 0);
    pnr_coverage c;
    const int rc = pnr_tree_coverage(ctx, T.xyz.data(), T.radius.data(), T.parent.data(), n, &job.opts, &c, job.per_node.empty() ? nullptr : vox.data(),
                                     job.per_node.empty() ? nullptr : fg.data(), job.per_node.empty() ? nullptr : sum.data(),
                                     job.mask.empty() ? nullptr : mask.data(), job.residual.empty() ? nullptr : residual.data());
    pnr_get_option(ctx, "render_items", &items);
    pnr_destroy(ctx);
    if (rc != PNR_OK) return lib_fail("pnr_tree_coverage");
    if (!job.mask.empty() && !write_stack(job.mask, mask, st.w, st.h, st.l)) return false;
    if (!job.residual.empty() && !write_stack(job.residual, residual, st.w, st.h, st.l)) return false;
    if (!job.per_node.empty()) {
        FILE *f = fopen(job.per_node.c_str(), "w");
        if (!f) {
            fprintf(stderr, "%s: cannot write the file\n", job.per_node.c_str());
            return false;
        }
        fprintf(f, "id,vox,fg,sum\n");
        for (size_t k = 0; k < (size_t)n; k++) fprintf(f, "%lld,%lld,%lld,%lld\n", T.id[k], (long long)vox[k], (long long)fg[k], (long long)sum[k]);
        if (fclose(f) != 0) {
            fprintf(stderr, "%s: write failed\n", job.per_node.c_str());
            return false;
        }
    }
    printf("{\"n_vox\": %lld, \"n_tree\": %lld, \"n_fg\": %lld, \"n_both\": %lld, \"sum_fg\": %lld, \"sum_both\": %lld, \"thr_used\": %d, \"covered\": %.17g, "
           "\"on_signal\": %.17g, \"covered_intensity\": %.17g, \"nodes\": %lld, \"items\": %lld}\n",
           (long long)c.n_vox, (long long)c.n_tree, (long long)c.n_fg, (long long)c.n_both, (long long)c.sum_fg, (long long)c.sum_both, (int)c.thr_used, c.covered,
           c.on_signal, c.covered_intensity, (long long)n, (long long)items);
    return true;
}

bool components_file(const ComponentsJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, float zscale, int device)
{
    auto lib_fail = [](const char *what) {
        fprintf(stderr, "%s: %s\n", what, pnr_last_error());
        return false;
    };
    const Settings &S = settings();
    Stack st;
    std::string err;
    if (!load_stack(infiles[0], raw_dims, st, err, S.channel - 1, S.raw_u16)) {
        fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
    if (S.windowed && st.bits != 16) {
        fprintf(stderr, "--window / --saturate need a 16-bit stack (8-bit input is never windowed)\n");
        return false;
    }
    pnr_params p;
    pnr_default_params(&p);
    if (zscale >= 1.f) p.zdist = zscale; // (the z half-width of --subtract-background)
    pnr_ctx *ctx = nullptr;
    if (pnr_create(&p, device, &ctx) != PNR_OK) return lib_fail("pnr_create");
    // the volume as it would be traced: windowed to 8 bits, then pre-filtered
    bool ok = (st.bits == 16 ? pnr_set_volume_u16(ctx, st.samples16(), st.w, st.h, st.l, 1, 0, S.windowed ? &S.window : nullptr, nullptr, nullptr)
                             : pnr_set_volume(ctx, st.bytes(), st.w, st.h, st.l)) == PNR_OK;
    if (ok && (S.filter.median || S.filter.tophat_r)) ok = pnr_filter_volume(ctx, &S.filter) == PNR_OK;
    if (!ok) {
        lib_fail("volume");
        pnr_destroy(ctx);
        return false;
    }
    const size_t N = (size_t)(st.w * st.h * st.l);
    std::vector<int32_t> labels(job.labels.empty() ? 0 : N);
    std::vector<pnr_component> comps;
    pnr_components_info ci = {};
    int rc = pnr_label_components(ctx, &job.opts, &ci, job.labels.empty() ? nullptr : labels.data(), nullptr, 0);
    if (rc == PNR_OK && !job.per_component.empty() && ci.n_comp > 0) { // "n_comp > cap: call again"
        comps.resize((size_t)ci.n_comp);
        rc = pnr_label_components(ctx, &job.opts, &ci, nullptr, comps.data(), (int64_t)comps.size());
    }
    pnr_destroy(ctx);
    if (rc != PNR_OK) return lib_fail("pnr_label_components");
    auto write_file = [](const std::string &name, const char *mode, const std::function<void(FILE *)> &body) {
        FILE *f = fopen(name.c_str(), mode);
        if (!f) {
            fprintf(stderr, "%s: cannot write the file\n", name.c_str());
            return false;
        }
        body(f);
        const bool bad = ferror(f) != 0;
        if (fclose(f) != 0 || bad) {
            fprintf(stderr, "%s: write failed\n", name.c_str());
            return false;
        }
        return true;
    };
    if (!job.labels.empty() && !write_file(job.labels, "wb", [&](FILE *f) { fwrite(labels.data(), 4, N, f); })) return false; // (the hosts this builds for are little-endian)
    if (!job.per_component.empty() && !write_file(job.per_component, "w", [&](FILE *f) {
            fprintf(f, "id,size,sum,cx,cy,cz,x0,y0,z0,x1,y1,z1,vmax\n");
            for (size_t k = 0; k < comps.size(); k++) {
                const pnr_component &c = comps[k];
                fprintf(f, "%lld,%lld,%lld,%.3f,%.3f,%.3f,%d,%d,%d,%d,%d,%d,%d\n", (long long)(k + 1), (long long)c.size, (long long)c.sum, (double)c.sx / (double)c.size,
                        (double)c.sy / (double)c.size, (double)c.sz / (double)c.size, c.x0, c.y0, c.z0, c.x1, c.y1, c.z1, c.vmax);
            }
        }))
        return false;
    printf("{\"n_vox\": %lld, \"n_fg\": %lld, \"n_comp\": %lld, \"n_small\": %lld, \"vox_small\": %lld, \"largest\": %lld, \"thr_used\": %d}\n", (long long)ci.n_vox,
           (long long)ci.n_fg, (long long)ci.n_comp, (long long)ci.n_small, (long long)ci.vox_small, (long long)ci.largest, (int)ci.thr_used);
    return true;
}

bool edt_file(const EdtJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, float zscale, int device)
{
    auto lib_fail = [](const char *what) {
        fprintf(stderr, "%s: %s\n", what, pnr_last_error());
        return false;
    };
    const Settings &S = settings();
    Stack st;
    std::string err;
    if (!load_stack(infiles[0], raw_dims, st, err, S.channel - 1, S.raw_u16)) {
        fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
    if (S.windowed && st.bits != 16) {
        fprintf(stderr, "--window / --saturate need a 16-bit stack (8-bit input is never windowed)\n");
        return false;
    }
    SwcTree T;
    if (!job.at.empty() && !load_swc(job.at, T, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
    pnr_params p;
    pnr_default_params(&p);
    p.zdist = zscale; // (also the z half-width of --subtract-background)
    pnr_ctx *ctx = nullptr;
    if (pnr_create(&p, device, &ctx) != PNR_OK) return lib_fail("pnr_create");
    // the volume as it would be traced: windowed to 8 bits, then pre-filtered
    bool ok = (st.bits == 16 ? pnr_set_volume_u16(ctx, st.samples16(), st.w, st.h, st.l, 1, 0, S.windowed ? &S.window : nullptr, nullptr, nullptr)
                             : pnr_set_volume(ctx, st.bytes(), st.w, st.h, st.l)) == PNR_OK;
    if (ok && (S.filter.median || S.filter.tophat_r)) ok = pnr_filter_volume(ctx, &S.filter) == PNR_OK;
    if (!ok) {
        lib_fail("volume");
        pnr_destroy(ctx);
        return false;
    }
    const size_t N = (size_t)(st.w * st.h * st.l);
    std::vector<float> d(job.out.empty() ? 0 : N), at((size_t)T.n());
    pnr_edt_info ei = {};
    const int rc = pnr_distance_transform(ctx, &job.opts, &ei, job.out.empty() ? nullptr : d.data(), T.n() ? T.xyz.data() : nullptr, T.n(), T.n() ? at.data() : nullptr);
    pnr_destroy(ctx);
    if (rc != PNR_OK) return lib_fail("pnr_distance_transform");
    auto write_file = [](const std::string &name, const char *mode, const std::function<void(FILE *)> &body) {
        FILE *f = fopen(name.c_str(), mode);
        if (!f) {
            fprintf(stderr, "%s: cannot write the file\n", name.c_str());
            return false;
        }
        body(f);
        const bool bad = ferror(f) != 0;
        if (fclose(f) != 0 || bad) {
            fprintf(stderr, "%s: write failed\n", name.c_str());
            return false;
        }
        return true;
    };
    for (float &v : d) v = sqrtf(v);
    if (!job.out.empty() && !write_file(job.out, "wb", [&](FILE *f) { fwrite(d.data(), 4, N, f); })) return false; // (the hosts this builds for are little-endian)
    if (!job.per_node.empty() && !write_file(job.per_node, "w", [&](FILE *f) {
            fprintf(f, "id,d\n");
            for (size_t k = 0; k < at.size(); k++) fprintf(f, "%lld,%.9g\n", T.id[k], (double)(at[k] < 0.f ? -1.f : sqrtf(at[k])));
        }))
        return false;
    printf("{\"n_vox\": %lld, \"n_fg\": %lld, \"n_capped\": %lld, \"thr_used\": %d, \"rmax\": %d, \"zdist\": %.17g, \"d_max\": %.17g, \"max_at\": ", (long long)ei.n_vox,
           (long long)ei.n_fg, (long long)ei.n_capped, (int)ei.thr_used, (int)job.opts.rmax, (double)zscale, (double)sqrtf(ei.d2_max));
    if (ei.first_max < 0) printf("null}\n");
    else printf("[%lld, %lld, %lld]}\n", (long long)(ei.first_max % st.w), (long long)(ei.first_max / st.w % st.h), (long long)(ei.first_max / (st.w * st.h)));
    return true;
}

bool geodesic_file(const GeodesicJob &job, const std::vector<char *> &infiles, const std::string &raw_dims, float zscale, int device)
{
    auto lib_fail = [](const char *what) {
        fprintf(stderr, "%s: %s\n", what, pnr_last_error());
        return false;
    };
    const Settings &S = settings();
    Stack st;
    std::string err;
    if (!load_stack(infiles[0], raw_dims, st, err, S.channel - 1, S.raw_u16)) {
        fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
    if (S.windowed && st.bits != 16) {
        fprintf(stderr, "--window / --saturate need a 16-bit stack (8-bit input is never windowed)\n");
        return false;
    }
    SwcTree A, B;
    if (!load_swc(job.from, A, err) || (!job.to.empty() && !load_swc(job.to, B, err))) {
        fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
    if (A.n() == 0) {
        fprintf(stderr, "%s: no nodes\n", job.from.c_str());
        return false;
    }
    for (long long id : A.id)
        if (id < 0 || id > 0x7fffffffLL) {
            fprintf(stderr, "%s: node id %lld is no label (0 .. 2147483647)\n", job.from.c_str(), id);
            return false;
        }
    // the sources: the sample points of the tree, labelled with their owner node's id
    int64_t ns = 0;
    if (pnr_tree_sample(A.xyz.data(), A.parent.data(), A.n(), 1.f, 1.f, nullptr, nullptr, 0, &ns) != PNR_OK) return lib_fail(job.from.c_str());
    std::vector<float> src((size_t)ns * 3);
    std::vector<int32_t> label((size_t)ns);
    if (pnr_tree_sample(A.xyz.data(), A.parent.data(), A.n(), 1.f, 1.f, src.data(), label.data(), ns, &ns) != PNR_OK) return lib_fail(job.from.c_str());
    for (int32_t &v : label) v = (int32_t)A.id[(size_t)v];
    pnr_params p;
    pnr_default_params(&p);
    p.zdist = zscale; // (also the z half-width of --subtract-background)
    pnr_ctx *ctx = nullptr;
    if (pnr_create(&p, device, &ctx) != PNR_OK) return lib_fail("pnr_create");
    // the volume as it would be traced: windowed to 8 bits, then pre-filtered
    bool ok = (st.bits == 16 ? pnr_set_volume_u16(ctx, st.samples16(), st.w, st.h, st.l, 1, 0, S.windowed ? &S.window : nullptr, nullptr, nullptr)
                             : pnr_set_volume(ctx, st.bytes(), st.w, st.h, st.l)) == PNR_OK;
    if (ok && (S.filter.median || S.filter.tophat_r)) ok = pnr_filter_volume(ctx, &S.filter) == PNR_OK;
    if (!ok) {
        lib_fail("volume");
        pnr_destroy(ctx);
        return false;
    }
    const size_t N = (size_t)(st.w * st.h * st.l);
    const int64_t m = B.n();
    std::vector<uint32_t> D(job.out.empty() ? 0 : N), d_at((size_t)m);
    std::vector<int32_t> L(job.out.empty() ? 0 : N), l_at((size_t)m), plen;
    std::vector<int64_t> pvox;
    pnr_geo_info gi = {};
    // the cap of the walks, fixed before the one call: a path visits a voxel at most once, no path has more than PNR_GEO_MAX_PATH voxels, and
    // all targets together get at most 2^26 entries (512 MB here and on the device)
    int32_t cap = 0;
    if (!job.paths.empty() && m) {
        cap = (int32_t)std::min<size_t>({(size_t)PNR_GEO_MAX_PATH, N, std::max<size_t>(64, ((size_t)1 << 26) / (size_t)m)});
        plen.resize((size_t)m), pvox.resize((size_t)m * (size_t)cap);
    }
    const int rc = pnr_geodesic_distance(ctx, src.data(), label.data(), ns, &job.opts, &gi, job.out.empty() ? nullptr : D.data(), job.out.empty() ? nullptr : L.data(),
                                         m ? B.xyz.data() : nullptr, m, m ? d_at.data() : nullptr, m ? l_at.data() : nullptr, cap, cap ? plen.data() : nullptr,
                                         cap ? pvox.data() : nullptr);
    pnr_destroy(ctx);
    if (rc != PNR_OK) return lib_fail("pnr_geodesic_distance");
    long long cut = 0;
    for (int32_t n : plen) cut += n < 0;
    if (cut) fprintf(stderr, "--paths: %lld path(s) of more than %d voxels are left out of %s\n", cut, (int)cap, job.paths.c_str());
    auto write_file = [](const std::string &name, const char *mode, const std::function<void(FILE *)> &body) {
        FILE *f = fopen(name.c_str(), mode);
        if (!f) {
            fprintf(stderr, "%s: cannot write the file\n", name.c_str());
            return false;
        }
        body(f);
        const bool bad = ferror(f) != 0;
        if (fclose(f) != 0 || bad) {
            fprintf(stderr, "%s: write failed\n", name.c_str());
            return false;
        }
        return true;
    };
    if (!job.out.empty()) { // (the hosts this builds for are little-endian)
        if (!write_file(job.out + "_d.raw", "wb", [&](FILE *f) { fwrite(D.data(), 4, N, f); })) return false;
        if (!write_file(job.out + "_label.raw", "wb", [&](FILE *f) { fwrite(L.data(), 4, N, f); })) return false;
    }
    if (!job.per_node.empty() && !write_file(job.per_node, "w", [&](FILE *f) {
            fprintf(f, "id,d,label\n");
            for (size_t k = 0; k < (size_t)m; k++) fprintf(f, "%lld,%lld,%d\n", B.id[k], d_at[k] == 0xffffffffu ? -1LL : (long long)d_at[k], (int)l_at[k]);
        }))
        return false;
    if (!job.paths.empty() && !write_file(job.paths, "w", [&](FILE *f) {
            long long next = 1;
            for (size_t k = 0; k < (size_t)m; k++) {
                const int32_t n = plen[k];
                if (n <= 0) continue; // (unreached, not finite, or cut at the cap: reported above)
                fprintf(f, "# path %lld -> %d: %d voxels, cost %u\n", B.id[k], (int)l_at[k], (int)n, (unsigned)d_at[k]);
                for (int32_t j = 0; j < n; j++) {
                    const long long v = pvox[k * (size_t)cap + (size_t)j];
                    fprintf(f, "%lld 2 %lld %lld %lld 1 %lld\n", next + j, v % st.w, v / st.w % st.h, v / (st.w * st.h), j + 1 < n ? next + j + 1 : -1LL);
                }
                next += n;
            }
        }))
        return false;
    printf("{\"n_vox\": %lld, \"n_pass\": %lld, \"n_reached\": %lld, \"n_src\": %lld, \"n_src_dropped\": %lld, \"thr_used\": %d, \"dmax\": %u, \"zdist\": %.17g, \"d_max\": %u, "
           "\"len_max\": %.17g, \"max_at\": ",
           (long long)gi.n_vox, (long long)gi.n_pass, (long long)gi.n_reached, (long long)gi.n_src, (long long)gi.n_src_dropped, (int)gi.thr_used, (unsigned)job.opts.dmax,
           (double)zscale, (unsigned)gi.d_max, (double)gi.d_max / 64.0);
    if (gi.first_max < 0) printf("null");
    else printf("[%lld, %lld, %lld]", (long long)(gi.first_max % st.w), (long long)(gi.first_max / st.w % st.h), (long long)(gi.first_max / (st.w * st.h)));
    printf(", \"rounds\": %d}\n", (int)gi.rounds);
    return true;
}

Stack::~Stack()
{
    if (view) munmap((void *)view, map_len);
}

std::vector<float> measured_radius_column(const std::vector<pnr_node> &tree, const std::vector<int32_t> &k)
{
    std::vector<float> r(tree.size(), -1.f);
    for (size_t i = 1; i < tree.size() && i < k.size(); i++)
        if (k[i] >= 0 && tree[i].type != 1) r[i] = k[i] >= 1 ? (float)k[i] : 0.5f;
    return r;
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
    FILE *f = fopen(swcname.c_str(), "w");
    if (!f) return false;
    if (!name.empty()) fprintf(f, "#name %s\n", name.c_str());
    if (!comment.empty()) {
        std::stringstream ss(comment);
        std::string ln;
        bool first = true;
        while (std::getline(ss, ln)) {
            if (ln.empty()) continue;
            fprintf(f, "%s%s\n", (first || ln[0] != '#') ? "#comment " : "", ln.c_str());
            first = false;
        }
    }
    fprintf(f, "##n,type,x,y,z,radius,parent\n");
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
    FILE *f = fopen(swcname.c_str(), "w");
    if (!f) return false;
    if (!name.empty()) fprintf(f, "#name %s\n", name.c_str());
    if (!comment.empty()) {
        std::stringstream ss(comment);
        std::string ln;
        bool first = true;
        while (std::getline(ss, ln)) {
            if (ln.empty()) continue;
            fprintf(f, "%s%s\n", (first || ln[0] != '#') ? "#comment " : "", ln.c_str());
            first = false;
        }
    }
    fprintf(f, "##n,type,x,y,z,radius,parent\n");
    for (size_t i = 1; i < tree.size(); i++) {
        const pnr_node &nd = tree[i];
        const float r = (radius && i < radius->size() && (*radius)[i] >= 0.f) ? (*radius)[i] : sig2r * nd.sig;
        fprintf(f, "%zu %d %.3f %.3f %.3f %.3f %d\n", i, (type == -1) ? nd.type : type, nd.x, nd.y, nd.z, r, parent[i]);
    }
    fclose(f);
    return true;
}

int parse_params(const std::vector<std::string> &paras, pnr_params &p, std::string &err)
{
    if ((int)paras.size() != nrInputParams) { // Advantra_plugin.cpp:295-299
        err = "Needs 11 input parameters.";
        return -1;
    }
    pnr_default_params(&p);
    { // parse_csv_string (:1885-1897): comma separated floats, sorted ascending
        std::vector<float> sig;
        std::stringstream ss(paras[0]);
        float v;
        while (ss >> v) {
            sig.push_back(v);
            if (ss.peek() == ',') ss.ignore();
        }
        std::sort(sig.begin(), sig.end());
        if (sig.empty() || sig.size() > PNR_MAX_SIGMAS) { err = "neuritesigmas out of range"; return -2; }
        p.nsig = (int)sig.size();
        for (int i = 0; i < p.nsig; i++) p.sig[i] = sig[i];
    }
    p.somaradius = atoi(paras[1].c_str());
    p.tolerance = (float)atof(paras[2].c_str());
    p.znccth = (float)atof(paras[3].c_str());
    p.kappa = (float)atof(paras[4].c_str());
    p.step = atoi(paras[5].c_str());
    p.ni = atoi(paras[6].c_str());
    p.np = atoi(paras[7].c_str());
    p.zdist = (float)atof(paras[8].c_str());
    p.nodepervol = atoi(paras[9].c_str());
    p.vol = atoi(paras[10].c_str());
    // range checks and messages of Advantra_plugin.cpp:317-326
    if (p.somaradius < 0) { err = "somaradius out of range"; return -2; }
    if (p.tolerance < 0) { err = "tolerance out of range"; return -2; }
    if (p.znccth < 0 || p.znccth > 1) { err = "znccth out of range"; return -2; }
    if (p.kappa < 0 || p.kappa > 5) { err = "kappa out of range"; return -2; }
    if (p.step < 1) { err = "step out of range"; return -2; }
    if (p.ni <= 0) { err = "ni out of range"; return -2; }
    if (p.np <= 0) { err = "np out of range"; return -2; }
    if (p.zdist < 1) { err = "zdist out of range"; return -2; }
    if (p.nodepervol <= 2 || p.nodepervol > 20) { err = "nodepervol out of range"; return -2; }
    if (!(p.vol == 1 || p.vol == 5 || p.vol == 9 || p.vol == 11 || p.vol == 19 || p.vol == 27)) { err = "vol can be 1,5,9,11,19,27"; return -2; }
    return 0;
}

// window: the (lo, hi) a 16-bit stack was windowed with (nullptr: 8-bit input); radius_thr: the threshold the radii were measured
// with (nullptr: not measured; 0: the relative mode)
// join: the result of a --join run (nullptr: not joined); cover: the result of a --mask / --residual / --coverage run (nullptr: none)
static std::string swc_comment(const std::vector<std::string> &paras, const pnr_params &p, const int32_t *window, const int32_t *radius_thr = nullptr,
                               const Result *join = nullptr, const Result *cover = nullptr)
{
    static const char *keys[] = {"neuritesigmas", "somaradius", "tolerance", "znccth", "kappa", "step", "ni", "np", "zdist", "nodepervol", "vol"};
    std::stringstream c;
    c << "email: miro@braincadet.com\n#params:\n#channel=" << settings().channel; // Advantra_plugin.cpp:2276-2306
    for (int i = 0; i < nrInputParams; i++) c << "\n#" << keys[i] << "=" << paras[i];
    c << "\n#------------------------\n#Kc=" << p.Kc << "\n#neff_ratio=" << p.neff_ratio << "\n#frangi_alfa=" << p.alpha
      << "\n#frangi_beta=" << p.beta << "\n#frangi_C=" << p.C << "\n#MAX_TRACE_COUNT=" << p.max_trace_count
      << "\n#EPSILON2=0.0001\n#REFINE_ITER=4\n#SIG2RADIUS=1.5\n#TRACE_RSMPL=1\n#GROUP_RADIUS=2\n#ENFORCE_SINGLE_TREE=0\n#TREE_SIZE_MIN=10\n#TAIL_SIZE_MIN=2";
    if (window) c << "\n#bits=16\n#window=" << window[0] << "," << window[1];
    const pnr_filter_opts &fo = settings().filter;
    if (fo.median || fo.tophat_r) {
        c << "\n#filter=median:" << (fo.median == 3 ? "3d" : fo.median == 2 ? "2d" : "off") << ",tophat:";
        if (fo.tophat_r) c << fo.tophat_r;
        else c << "off";
    }
    if (settings().despeckle && cover)
        c << "\n#despeckle=min:" << settings().despeckle_opts.min_size << ",thr:" << cover->despeckle_thr << ",conn:" << settings().despeckle_opts.connectivity
          << ",removed:" << cover->despeckle_removed << ",voxels:" << cover->despeckle_voxels;
    if (join) c << "\n#join=gap:" << f32_text(settings().join_gap) <<",bridges:" << join->join_bridges << ",trees:" << join->join_trees_in << "->" << join->join_trees_out;
    if (radius_thr) {
        const pnr_radius_opts &ro = settings().radius;
        c << "\n#radius=measured,thr=";
        if (ro.rel_pct > 0) c << "rel:" << ro.rel_pct;
        else c << *radius_thr;
        c << ",rmax=" << ro.rmax << ",bg=" << ro.bg_permille;
    }
    if (cover && cover->have_coverage) {
        char buf[200];
        snprintf(buf, sizeof buf, "\n#coverage=thr:%d,covered:%.6f,on_signal:%.6f,intensity:%.6f,tree_voxels:%lld", (int)cover->coverage.thr_used, cover->coverage.covered,
                 cover->coverage.on_signal, cover->coverage.covered_intensity, (long long)cover->coverage.n_tree);
        c << buf;
    }
    return c.str();
}

bool advantra_func(const std::vector<char *> &infiles, const std::vector<char *> &paras_c, int device, const std::string &raw_dims,
                   Result *result)
{
    if (infiles.empty()) {
        fprintf(stderr, "Need input image. \n"); // :286-289
        return false;
    }
    std::vector<std::string> paras(paras_c.begin(), paras_c.end());
    pnr_params p;
    std::string err;
    const int pr = parse_params(paras, p, err);
    if (pr == -1) {
        fprintf(stderr, "\nNeeds %d input parameters.\n\n", nrInputParams);
        print_help();
        return false;
    }
    if (pr == -2) {
        fprintf(stderr, "%s\n", err.c_str()); // v3d_msg(...); return 0
        return true;
    }
    Stack st;
    const auto tl0 = std::chrono::steady_clock::now();
    const Settings &S = settings();
    if (!load_stack(infiles[0], raw_dims, st, err, S.channel - 1, S.raw_u16)) {
        fprintf(stderr, "%s\n", err.c_str());
        return true;
    }
    if (S.windowed && st.bits != 16) { // 8-bit input is taken as it is, as the reference does
        fprintf(stderr, "--window / --saturate need a 16-bit stack (8-bit input is never windowed)\n");
        return false;
    }
    Result local;
    Result *R = result ? result : &local;
    const double t_load = std::chrono::duration<double>(std::chrono::steady_clock::now() - tl0).count();
    // a failure of the device library (no GPU, out of memory, a failed exchange) has no counterpart in the reference's contract:
    // it is reported on stderr by reconstruction_func and makes the function -- and the CLI's exit status -- fail
    const uint16_t *deep = st.bits == 16 ? st.samples16() : nullptr;
    if (!reconstruction_func(deep ? nullptr : st.bytes(), st.w, st.h, st.l, infiles[0], paras, p, device, R, deep, S.windowed ? &S.window : nullptr))
        return false;
    if (settings().rank == 0) {
        // what a user of advantra_func waits for (Advantra_plugin.cpp:2241 load, :2183-2731 reconstruction_func, :2164 the SWC)
        R->t_load = t_load;
        R->t_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - tl0).count();
        printf("wall: load %.3f s, context + upload %.3f s, frangi %.3f s, seeds %.3f s, selection %.3f s, tracing %.3f s, reconstruct %.3f s, "
               "write %.3f s | total %.3f s for %lld voxels\n",
               R->t_load, R->t_setup, R->t_frangi, R->t_seeds, R->t_select, R->t_trace, R->t_recon, R->t_write, R->t_total, (long long)(st.w * st.h * st.l));
    }
    return true;
}

// ---- the few collectives of the sharded path, over the transport the ranks were joined with: the shared-memory all-gather of the
// ranks of this host (default) or RCCL (--exchange rccl) -----------------------------------------------------------------------------
namespace {
constexpr size_t XCHUNK = 1 << 18; // bytes per rank and call (both transports are opened with this capacity)
bool allgather_bytes(pnr_allgather_fn fn, void *user, int world, const void *send, size_t n, std::vector<unsigned char> &out)
{
    out.assign(n * (size_t)world, 0);
    std::vector<unsigned char> sb(XCHUNK), rb(XCHUNK * (size_t)world);
    for (size_t off = 0; off < n || off == 0; off += XCHUNK) {
        const size_t m = std::min(XCHUNK, n - off);
        if (m) std::memcpy(sb.data(), (const unsigned char *)send + off, m);
        if (fn(user, sb.data(), rb.data(), (int64_t)m) != PNR_OK) return false;
        for (int r = 0; r < world; r++)
            if (m) std::memcpy(out.data() + (size_t)r * n + off, rb.data() + (size_t)r * m, m);
        if (n == 0) break;
    }
    return true;
}
} // namespace

bool reconstruction_func(const unsigned char *data1d, long long w, long long h, long long l, const std::string &inimg_file,
                         const std::vector<std::string> &paras, pnr_params p, int device, Result *result, const uint16_t *data16,
                         const pnr_window *win)
{
    const int rank = settings().rank, world = settings().world;
    // the transport of the sharded path's collectives
    pnr_rccl_exchange *const RX = settings().rccl;
    const pnr_allgather_fn xfn = RX ? pnr_rccl_allgather : pnr_shm_allgather;
    void *const X = RX ? (void *)RX : (void *)settings().exchange;
    const bool sharded = world > 1 || settings().force_shard;
    if (sharded && (!X || l < 2)) {
        fprintf(stderr, "--ranks needs a stack of at least 2 planes and an open exchange\n");
        return false;
    }
    if (rank != 0) { // only rank 0 talks
        if (!freopen("/dev/null", "w", stdout)) return false;
    }
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    p.rng_seed = settings().rng_seed;
    printf("-------------  ADVANTRA  -------------\n");
    const auto t_begin = clk::now();
    pnr_ctx *ctx = nullptr;
    if (pnr_create(&p, device, &ctx) != PNR_OK) {
        fprintf(stderr, "%s\n", pnr_last_error());
        return false;
    }
    pnr_set_option(ctx, "local_ranks", world);
    const auto t_created = clk::now();
    Result R;
    bool ok = true;
    auto run_soma = [&]() { // SOMA EXTR. (:2426-2486): erosion, xy blur, max-entropy threshold, regions -> soma nodes
        if (p.somaradius <= 0) { printf("no soma detection\n"); return; }
        auto ts = clk::now();
        int32_t th = 0;
        int64_t nsoma = 0;
        ok = ok && pnr_soma(ctx, nullptr, &th, &nsoma) == PNR_OK;
        printf("imerode(%d) imgaussian(%d) maxentropy_th() %d  %lld soma regions  %.3f sec.\n", p.somaradius, p.somaradius, (int)th, (long long)nsoma,
               std::chrono::duration<double>(clk::now() - ts).count());
    };
    const pnr_filter_opts &fo = settings().filter;
    const bool despeckled = settings().despeckle;
    const bool filtered = fo.median || fo.tophat_r || despeckled;
    auto run_despeckle = [&]() { // --despeckle: the small foreground components of the (filtered) volume are cleared
        if (!despeckled || !ok) return;
        const auto tf = clk::now();
        pnr_components_info ci = {};
        ok = pnr_despeckle_volume(ctx, &settings().despeckle_opts, &ci) == PNR_OK;
        R.t_despeckle = std::chrono::duration<double>(clk::now() - tf).count();
        R.despeckle_removed = ci.n_small, R.despeckle_voxels = ci.vox_small, R.despeckle_thr = ci.thr_used;
        printf("despeckle... %lld components of fewer than %lld voxels (%lld voxels) removed, threshold %d, %g sec.\n", (long long)ci.n_small,
               (long long)settings().despeckle_opts.min_size, (long long)ci.vox_small, (int)ci.thr_used, R.t_despeckle);
        if (settings().timing) fprintf(stderr, "[pnr host] despeckle: %.3f s\n", R.t_despeckle);
    };
    auto run_filter = [&]() { // --median / --subtract-background (/ --despeckle): the context's volume is replaced by its filtered bytes
        if (!filtered || !ok) return;
        if (!fo.median && !fo.tophat_r) return run_despeckle();
        const auto tf = clk::now();
        const bool prof = settings().timing || settings().verbose;
        if (prof) pnr_set_profiling(ctx, 1);
        ok = pnr_filter_volume(ctx, &fo) == PNR_OK;
        R.t_filter = std::chrono::duration<double>(clk::now() - tf).count();
        double ms = 0;
        int64_t launches = 0;
        if (prof) {
            pnr_get_kernel_ms(ctx, "filter", &ms, &launches);
            pnr_set_profiling(ctx, 0);
        }
        printf("pre-filter... median %s, top-hat %d, %g sec.\n", fo.median == 3 ? "3d" : fo.median == 2 ? "2d" : "off", (int)fo.tophat_r, R.t_filter);
        if (settings().verbose) printf("pre-filter kernels %.3f ms in %lld launches\n", ms, (long long)launches);
        if (settings().timing) fprintf(stderr, "[pnr host] filter: %.3f s, kernels %.3f ms in %lld launches\n", R.t_filter, ms, (long long)launches);
        run_despeckle();
    };
    std::vector<pnr_seed> seeds;
    int64_t nfound = 0, nseeds = 0;
    auto t0 = clk::now(), t1 = t0, t2 = t0;
    int32_t window[2] = {-1, -1}; // 16-bit input: the window it was mapped with
    std::vector<unsigned char> mapped;
    if (!sharded) {
        ok = (data16 ? pnr_set_volume_u16(ctx, data16, w, h, l, 1, 0, win, &window[0], &window[1]) : pnr_set_volume(ctx, data1d, w, h, l)) == PNR_OK;
        if (settings().timing) fprintf(stderr, "[pnr host] context %.3f s, upload of %.2f GB %.3f s\n", secs(t_begin, t_created), (double)(w * h * l) / 1e9, secs(t_created, clk::now()));
        run_filter();
        if (ok) run_soma();
        t0 = clk::now();
        ok = ok && pnr_frangi(ctx, &R.Jmin, &R.Jmax) == PNR_OK; // :2496-2512
        t1 = clk::now();
        const pnr_seed *found = nullptr;
        ok = ok && pnr_extract_seeds(ctx, &found, &nfound) == PNR_OK; // :2549
        t2 = clk::now();
        if (ok) {
            seeds.assign(found, found + nfound);
            printf("seed extraction... %gk seeds,  %g sec.\n", nfound / 1000.0, secs(t1, t2));
            ok = pnr_score_filter_sort_seeds(ctx, seeds.data(), nfound, &nseeds) == PNR_OK; // :2561-2586
            seeds.resize((size_t)nseeds);
        }
    } else {
        if (data16) { // every rank maps the whole stack once and runs the 8-bit path on it: slabs and stack share one window
            mapped.resize((size_t)(w * h * l));
            ok = pnr_set_volume_u16(ctx, data16, w, h, l, 1, 0, win, &window[0], &window[1]) == PNR_OK && pnr_get_volume(ctx, mapped.data()) == PNR_OK;
            data1d = mapped.data();
        }
        if (filtered) { // every rank filters its own copy of the whole stack (the filter is deterministic: all ranks hold the same bytes)
            if (!data16) ok = pnr_set_volume(ctx, data1d, w, h, l) == PNR_OK;
            run_filter();
            mapped.resize((size_t)(w * h * l));
            ok = ok && pnr_get_volume(ctx, mapped.data()) == PNR_OK;
            data1d = mapped.data();
        }
        // this rank's z-slab with its halo (the z pass of the widest Gaussian + the radius-2 Hessian stencil): exact Frangi / seeds
        // of the planes it owns, no halo exchange -- every rank has the whole stack
        float smax = 0;
        for (int i = 0; i < p.nsig; i++) smax = std::max(smax, p.sig[i]);
        const long long halo = (long long)std::ceil(3 * (smax / p.zdist)) + 2;
        const long long z0 = l * rank / world, z1 = l * (rank + 1) / world, zlo = std::max(0LL, z0 - halo), zhi = std::min(l, z1 + halo);
        float mm[2] = {FLT_MAX, -FLT_MAX}; // (min, max) of J over the owned planes
        const pnr_seed *found = nullptr;
        int64_t nmine = 0;
        std::vector<pnr_seed> mine;
        if (z1 > z0) {
            ok = ok && pnr_set_volume(ctx, data1d + zlo * w * h, w, h, zhi - zlo) == PNR_OK;
            ok = ok && pnr_frangi_slab(ctx, z0 - zlo, z1 - zlo, &mm[0], &mm[1]) == PNR_OK;
        }
        // the 2-float all-reduce: one ncclAllReduce over RCCL, an all-gather + local reduction through shared memory
        R.Jmin = FLT_MAX; R.Jmax = -FLT_MAX;
        if (RX) {
            R.Jmin = mm[0]; R.Jmax = mm[1];
            if (pnr_rccl_allreduce_minmax(RX, &R.Jmin, &R.Jmax) != PNR_OK) ok = false;
        } else {
            std::vector<unsigned char> all;
            if (!allgather_bytes(xfn, X, world, mm, sizeof(mm), all)) ok = false;
            for (int r = 0; r < world && ok; r++) {
                float q[2];
                std::memcpy(q, all.data() + (size_t)r * sizeof(q), sizeof(q));
                R.Jmin = std::min(R.Jmin, q[0]); R.Jmax = std::max(R.Jmax, q[1]);
            }
        }
        t1 = clk::now();
        if (ok && z1 > z0) {
            ok = pnr_quantise_j8(ctx, R.Jmin, R.Jmax) == PNR_OK && pnr_extract_seeds_range(ctx, z0 - zlo, z1 - zlo, &found, &nmine) == PNR_OK;
            if (ok) {
                mine.assign(found, found + nmine);
                for (auto &sd : mine) sd.z += (float)zlo;
            }
        }
        t2 = clk::now();
        ok = ok && pnr_set_volume(ctx, data1d, w, h, l) == PNR_OK; // scoring and tracing see the whole stack
        if (ok) run_soma();
        int64_t cnt[2] = {nmine, 0};
        if (ok && nmine) ok = pnr_score_filter_seeds(ctx, mine.data(), nmine, &cnt[1]) == PNR_OK; // this slab's seeds: znccBBB + threshold
        if (!ok) cnt[0] = -1; // a rank that failed says so: every collective up to here was entered by everybody, none after is
        std::vector<unsigned char> counts;
        if (!allgather_bytes(xfn, X, world, cnt, sizeof(cnt), counts)) ok = false;
        int64_t mx = 0;
        std::vector<int64_t> kept((size_t)world);
        for (int r = 0; r < world; r++) {
            int64_t q[2] = {-1, 0};
            if (counts.size() >= (size_t)(r + 1) * sizeof(q)) std::memcpy(q, counts.data() + (size_t)r * sizeof(q), sizeof(q));
            if (q[0] < 0) { if (ok) fprintf(stderr, "rank %d failed\n", r); ok = false; continue; }
            nfound += q[0]; kept[(size_t)r] = q[1]; mx = std::max(mx, q[1]);
        }
        mine.resize((size_t)mx); // padded payloads
        std::vector<unsigned char> pay;
        if (ok && !allgather_bytes(xfn, X, world, mine.data(), (size_t)mx * sizeof(pnr_seed), pay)) ok = false;
        for (int r = 0; r < world && ok; r++) { // rank order = the z-major order of the unsharded extraction
            const pnr_seed *q = (const pnr_seed *)(pay.data() + (size_t)r * (size_t)mx * sizeof(pnr_seed));
            seeds.insert(seeds.end(), q, q + kept[(size_t)r]);
        }
        if (ok) {
            printf("seed extraction... %gk seeds,  %g sec.\n", nfound / 1000.0, secs(t1, t2));
            nseeds = (int64_t)seeds.size();
            if (nseeds) ok = pnr_sort_seeds(ctx, seeds.data(), nseeds, &nseeds) == PNR_OK; // the list one GPU would have
            seeds.resize((size_t)nseeds);
        }
    }
    auto t3 = clk::now();
    int64_t nn = 0, nl = 0, used = 0, iters = 0;
    if (ok) {
        printf("seed selection & sorting... %gk seeds, %g sec.\ntracing...\n", nseeds / 1000.0, secs(t2, t3));
        // :2658-2710: the particle filters on the GPU (a window of traces refilled as they stop), the bookkeeping replayed on the
        // host in seed order; the graph stays in the context and is fetched once its size is known
        if (settings().verbose) pnr_set_option(ctx, "trace_log", 1);
        if (settings().timing) { pnr_set_option(ctx, "trace_timing", 1); pnr_set_option(ctx, "recon_timing", 1); }
        if (!sharded)
            ok = pnr_trace_replay(ctx, seeds.data(), nseeds, 0, nullptr, 0, &nn, nullptr, 0, &nl, &used, &iters) == PNR_OK;
        else // every rank traces seeds rank, rank + world, ...; finished traces are exchanged and replayed in seed order on every rank
            ok = pnr_trace_replay_sharded(ctx, seeds.data(), nseeds, rank, world, xfn, X, nullptr, 0, &nn, nullptr, 0, &nl, &used, &iters) == PNR_OK;
        if (ok) {
            R.nodes.resize((size_t)nn);
            R.links.resize((size_t)(2 * nl));
            ok = pnr_get_graph(ctx, R.nodes.data(), nn, &nn, R.links.data(), nl, &nl) == PNR_OK;
        }
        if (ok && settings().verbose) { // what the reference prints while it traces (TRACING_VERBOSE :2677; tracker.cpp:866,879,908,916)
            int64_t nlog = 0;
            pnr_get_trace_log(ctx, nullptr, 0, &nlog);
            std::vector<int32_t> lg((size_t)nlog * 5);
            pnr_get_trace_log(ctx, lg.data(), nlog, &nlog);
            int trace_count = 0;
            for (int64_t k = 0; k < nlog; k++) {
                const int32_t *e = &lg[(size_t)k * 5];
                const pnr_seed &sd = seeds[(size_t)e[0]];
                if (e[1] == 0)
                    printf("\nTrace: %6d\t [%4.1f, %4.1f, %4.1f]\t sc=%6.2f\t corr=%3.2f\t progress %3.2f%%\t", ++trace_count, sd.x, sd.y, sd.z, sd.score, sd.corr,
                           (100.0 * e[0]) / (double)nseeds);
                float cv;
                std::memcpy(&cv, &e[4], 4);
                switch (e[3]) {
                case 3: printf("\n--%d[%d], SOMA, idx=%d", e[2], p.ni, e[4]); break;
                case 2: printf("\n--%d[%d], DENSITY, nodespervol=%d", e[2], p.ni, e[4]); break;
                case 1: printf("\n--%d[%d], success=0, corr=%1.2f", e[2], p.ni, cv); break;
                default: printf("\n--%d[%d], TRACK LIMIT, niter=%d", e[2], p.ni, p.ni); break;
                }
            }
            printf("\n");
        }
    }
    auto t4 = clk::now();
    if (!ok) {
        fprintf(stderr, "%s\n", pnr_last_error());
        pnr_destroy(ctx);
        return false;
    }
    R.n_seeds_init = nfound; R.n_seeds = nseeds; R.n_traces = used; R.n_iterations = iters;
    if (rank != 0) { // every rank holds the same graph; rank 0 post-processes and writes it
        pnr_destroy(ctx);
        if (result) *result = R;
        return true;
    }
    R.t_frangi = secs(t0, t1); R.t_seeds = secs(t1, t2); R.t_select = secs(t2, t3); R.t_trace = secs(t3, t4);
    R.t_setup = secs(t_begin, t0); // context, upload of the stack, soma path
    printf("\n-----\n%g%% seeds used \n", nseeds ? 100.0 * used / nseeds : 0.0);
    { // reconstruct(n0, ...) :2729 -> :2096-2181: refinement and grouping queries on this rank's GPU, trees and resampling on the host
        int64_t cap = std::max<int64_t>(16, 4 * nn), nt = 0;
        for (;;) {
            R.tree.resize((size_t)cap);
            R.parent.resize((size_t)cap);
            if (pnr_reconstruct_ctx(ctx, R.nodes.data(), nn, R.links.data(), nl, 0, 0, 0, 0, 0, settings().single_tree ? -1 : 0, R.tree.data(), R.parent.data(), cap, &nt) != PNR_OK) {
                fprintf(stderr, "%s\n", pnr_last_error());
                pnr_destroy(ctx);
                return false;
            }
            if (nt <= cap) break;
            cap = nt;
        }
        R.tree.resize((size_t)nt);
        R.parent.resize((size_t)nt);
    }
    if (settings().join && R.tree.size() > 1) { // --join: the forest becomes one tree (pnr_join_trees), the tree list is rewritten in tree order
        const auto tj = clk::now();
        const Settings &S = settings();
        const int64_t n = (int64_t)R.tree.size() - 1; // without the dummy
        std::vector<float> xyz((size_t)(3 * n));
        std::vector<int32_t> par((size_t)n), par_out((size_t)n), order((size_t)n), comp((size_t)n);
        int64_t root = -1;
        for (int64_t i = 0; i < n; i++) {
            const pnr_node &nd = R.tree[(size_t)i + 1];
            xyz[(size_t)(3 * i)] = nd.x, xyz[(size_t)(3 * i + 1)] = nd.y, xyz[(size_t)(3 * i + 2)] = nd.z;
            par[(size_t)i] = R.parent[(size_t)i + 1] > 0 ? R.parent[(size_t)i + 1] - 1 : -1;
            if (S.join_root_id == 0 && root < 0 && nd.type == 1) root = i; // the first soma node
        }
        if (S.join_root_id > 0) root = S.join_root_id - 1;
        if (root >= n) {
            fprintf(stderr, "--join-root %lld: the tree has %lld nodes\n", S.join_root_id, (long long)n);
            pnr_destroy(ctx);
            return false;
        }
        const pnr_join_opts jo = {p.zdist, S.join_gap, (int32_t)root};
        int64_t nb = 0, t_in = 0, t_out = 0;
        if (S.timing) pnr_set_profiling(ctx, 1);
        if (pnr_join_trees(ctx, xyz.data(), par.data(), n, &jo, par_out.data(), order.data(), comp.data(), nullptr, 0, &nb, &t_in, &t_out) != PNR_OK) {
            fprintf(stderr, "%s\n", pnr_last_error());
            pnr_destroy(ctx);
            return false;
        }
        R.join_bridges = nb, R.join_trees_in = t_in, R.join_trees_out = t_out;
        std::vector<int32_t> pos((size_t)n, -1); // node -> its line; component 0 comes first in the order
        std::vector<pnr_node> tree(1, R.tree[0]);
        std::vector<int32_t> parent(1, R.parent[0]);
        for (int64_t k = 0; k < n; k++) {
            const int32_t v = order[(size_t)k];
            if (S.join_keep_largest && comp[(size_t)v] != 0) break;
            pos[(size_t)v] = (int32_t)tree.size();
            tree.push_back(R.tree[(size_t)v + 1]);
            parent.push_back(par_out[(size_t)v] < 0 ? -1 : pos[(size_t)par_out[(size_t)v]]); // (the parent was written before)
        }
        R.tree.swap(tree);
        R.parent.swap(parent);
        R.t_join = secs(tj, clk::now());
        printf("join... gap %g, %lld bridges, %lld -> %lld trees, %zu nodes written, %g sec.\n", (double)S.join_gap, (long long)nb, (long long)t_in, (long long)t_out,
               R.tree.size() - 1, R.t_join);
        if (S.timing) {
            double ms = 0;
            int64_t launches = 0, rounds = 0;
            pnr_get_kernel_ms(ctx, "join", &ms, &launches);
            pnr_get_option(ctx, "join_rounds", &rounds);
            pnr_set_profiling(ctx, 0);
            fprintf(stderr, "[pnr host] join: %.3f s, %lld rounds, kernels %.3f ms in %lld launches\n", R.t_join, (long long)rounds, ms, (long long)launches);
        }
    }
    auto t5 = clk::now();
    R.t_recon = secs(t4, t5);
    std::vector<float> radius; // --measure-radius: the radius column, measured on the volume this context traced
    if (settings().measure_radius) {
        const size_t nt = R.tree.size();
        std::vector<float> xyz(3 * nt, 0.f);
        for (size_t i = 0; i < nt; i++) { xyz[3 * i] = R.tree[i].x; xyz[3 * i + 1] = R.tree[i].y; xyz[3 * i + 2] = R.tree[i].z; }
        R.radius_k.assign(nt, -1);
        if (settings().timing) pnr_set_profiling(ctx, 1);
        if (pnr_measure_radii(ctx, xyz.data(), (int64_t)nt, &settings().radius, R.radius_k.data(), &R.radius_thr) != PNR_OK) {
            fprintf(stderr, "%s\n", pnr_last_error());
            pnr_destroy(ctx);
            return false;
        }
        if (nt) R.radius_k[0] = -1; // the dummy
        radius = measured_radius_column(R.tree, R.radius_k);
        t5 = clk::now();
        R.t_radius = secs(t4, t5) - R.t_recon;
        printf("radius measurement... %zu nodes, %g sec.\n", nt ? nt - 1 : 0, R.t_radius);
        if (settings().timing) {
            double ms = 0;
            int64_t launches = 0;
            pnr_get_kernel_ms(ctx, "radius", &ms, &launches);
            fprintf(stderr, "[pnr host] radius: %.3f s, kernels %.3f ms in %lld launches\n", R.t_radius, ms, (long long)launches);
        }
    }
    if (!settings().mask_out.empty() || !settings().residual_out.empty() || settings().coverage) { // the final tree rendered on the traced volume
        const auto tr = clk::now();
        const Settings &S = settings();
        const int64_t n = (int64_t)R.tree.size() - 1; // without the dummy
        std::vector<float> xyz((size_t)(3 * std::max<int64_t>(n, 0))), rad((size_t)std::max<int64_t>(n, 0));
        std::vector<int32_t> par((size_t)std::max<int64_t>(n, 0));
        for (int64_t i = 0; i < n; i++) {
            const pnr_node &nd = R.tree[(size_t)i + 1];
            xyz[(size_t)(3 * i)] = nd.x, xyz[(size_t)(3 * i + 1)] = nd.y, xyz[(size_t)(3 * i + 2)] = nd.z;
            par[(size_t)i] = R.parent[(size_t)i + 1] > 0 ? R.parent[(size_t)i + 1] - 1 : -1;
            rad[(size_t)i] = (!radius.empty() && radius[(size_t)i + 1] >= 0.f) ? radius[(size_t)i + 1] : 1.f * nd.sig; // what save_treelist writes
        }
        const size_t N = (size_t)(w * h * l);
        std::vector<unsigned char> mask(S.mask_out.empty() ? 0 : N), residual(S.residual_out.empty() ? 0 : N);
        const pnr_render_opts ro = {p.zdist, 1.f, 0.f, -1};
        if (S.timing) pnr_set_profiling(ctx, 1);
        std::string werr;
        bool rok = pnr_tree_coverage(ctx, xyz.data(), rad.data(), par.data(), std::max<int64_t>(n, 0), &ro, &R.coverage, nullptr, nullptr, nullptr,
                                     S.mask_out.empty() ? nullptr : mask.data(), S.residual_out.empty() ? nullptr : residual.data()) == PNR_OK;
        if (!rok) werr = pnr_last_error();
        rok = rok && (S.mask_out.empty() || save_stack_u8(S.mask_out, mask.data(), w, h, l, werr));
        rok = rok && (S.residual_out.empty() || save_stack_u8(S.residual_out, residual.data(), w, h, l, werr));
        if (!rok) {
            fprintf(stderr, "%s\n", werr.c_str());
            pnr_destroy(ctx);
            return false;
        }
        R.have_coverage = true;
        R.t_render = secs(tr, clk::now());
        printf("render... %lld tree voxels, covered %.4f, on signal %.4f, intensity %.4f (threshold %d), %g sec.\n", (long long)R.coverage.n_tree, R.coverage.covered,
               R.coverage.on_signal, R.coverage.covered_intensity, (int)R.coverage.thr_used, R.t_render);
        if (S.timing) {
            double ms = 0;
            int64_t launches = 0;
            pnr_get_kernel_ms(ctx, "render", &ms, &launches);
            pnr_set_profiling(ctx, 0);
            fprintf(stderr, "[pnr host] render: %.3f s, kernels %.3f ms in %lld launches\n", R.t_render, ms, (long long)launches);
        }
        t5 = clk::now();
    }
    R.swc_path = inimg_file + (settings().single_tree ? "_Advantra1.swc" : "_Advantra.swc"); // :2152 / :2164
    save_treelist(R.tree, R.parent, R.swc_path, -1, 1.f, "Advantra",
                  swc_comment(paras, p, data16 ? window : nullptr, settings().measure_radius ? &R.radius_thr : nullptr, settings().join ? &R : nullptr, &R),
                  radius.empty() ? nullptr : &radius);
    if (settings().save_midres) { // the saveMidres taps of reconstruct() (:2098-2141)
        save_nodelist(R.nodes, R.links, inimg_file + "_n0_.swc");
        static const char *const names[] = {"", "_n0res_.swc", "_n1_.swc", "_n2_.swc", "_n2tree_.swc"};
        for (int stage = 1; stage <= 4; stage++) {
            int64_t sn = 0, sl = 0;
            if (pnr_reconstruct_stage(R.nodes.data(), nn, R.links.data(), nl, 0, 0, 0, 0, 0, stage, nullptr, 0, &sn, nullptr, 0, &sl) != PNR_OK) break;
            std::vector<pnr_node> tn((size_t)sn);
            std::vector<int32_t> tl((size_t)(2 * sl));
            if (pnr_reconstruct_stage(R.nodes.data(), nn, R.links.data(), nl, 0, 0, 0, 0, 0, stage, tn.data(), sn, &sn, tl.data(), sl, &sl) != PNR_OK) break;
            if (stage < 4) save_nodelist(tn, tl, inimg_file + names[stage]);
            else { // a tree list: every node carries its parent (or none)
                std::vector<int32_t> par((size_t)sn, -1);
                for (int64_t k = 0; k < sl; k++) par[(size_t)tl[(size_t)(2 * k)]] = tl[(size_t)(2 * k + 1)];
                save_treelist(tn, par, inimg_file + names[stage], -1, 1.f, "", "");
            }
        }
    }
    R.t_write = secs(t5, clk::now());
    printf("%s\n%lld trace nodes, %lld traces, %lld SMC iterations, %zu tree nodes | frangi %.3f s, seeds %.3f s, selection %.3f s, "
           "tracing %.3f s, reconstruct %.3f s\n",
           R.swc_path.c_str(), (long long)nn - 1, (long long)used, (long long)iters, R.tree.size() - 1, R.t_frangi, R.t_seeds, R.t_select,
           R.t_trace, R.t_recon);
    pnr_destroy(ctx);
    if (result) *result = R;
    return true;
}

} // namespace advantra
