// stack_reader.cpp -- the host's stack reader (see advantra_host.h): load_stack, --info, and the load every run of the CLI starts
// with.  stack_io.cpp, the writer, is apart from it because the device library compiles that file too.
#include "host_internal.h"
#include <algorithm>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <cstdlib>
#include <cstring>
#include <fstream>

namespace advantra {

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

Loaded load_input_stack(const std::string &path, const std::string &raw_dims, Stack &out)
{
    const Settings &S = settings();
    std::string err;
    if (!load_stack(path, raw_dims, out, err, S.channel - 1, S.raw_u16)) {
        fprintf(stderr, "%s\n", err.c_str());
        return Loaded::unreadable;
    }
    if (S.windowed && out.bits != 16) { // 8-bit input is taken as it is, as the reference does
        fprintf(stderr, "--window / --saturate need a 16-bit stack (8-bit input is never windowed)\n");
        return Loaded::not_windowable;
    }
    return Loaded::ok;
}

Stack::~Stack()
{
    if (view) munmap((void *)view, map_len);
}

} // namespace advantra
