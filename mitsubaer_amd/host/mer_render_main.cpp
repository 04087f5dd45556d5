// mer_render -- minimal driver over the C++ host mirror:  mer_render [-D key=value]... [-s spp] [-o out.npy] [--gpus N | --devices a,b,..] [--tiles] [--mesh-sdf[=N]] [--ordered] [--fluence=NX,NY,NZ [--time-resolved | --track-length]] [--exitance=NU,NV [--time-resolved] [--accept-cos=C]] [--frequencies=K1[,K2,...]] [--sensitivity=NX,NY,NZ --detector=FACE,NU,NV,IU0,IU1,IV0,IV1 [--accept-cos=C] [--gate=TMIN,TBIN] [--detector-bins=BU,BV] [--gates=N] [--scatter]] scene.xml
// (the reference's `mitsuba` CLI, src/mitsuba/mitsuba.cpp:154-246, reduced to what the hot path needs)
#include "mer_host.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// the window of --time-resolved: the film's transient window (minBound, binWidth, ceil((maxBound - minBound) / binWidth) frames)
struct Window { int frames; float tMin, tBin; };
static Window filmWindow(const merhost::Scene &scene) {
    const merhost::Film &film = *scene.sensor->film;
    if (film.decomposition != MER_DECOMPOSITION_TRANSIENT) merhost::Log_EError("--time-resolved takes its window from the film: the film needs decomposition = transient");
    return {(int) std::ceil((film.maxBound - film.minBound) / film.binWidth), film.minBound, film.binWidth};
}
// a VOL of cell values: its box is that of the cell centres, so that a gridvolume reading it interpolates between them
static void writeCellVol(const std::string &path, const std::vector<float> &v, const int res[3], const float bmin[3], const float bmax[3]) {
    float lo[3], hi[3];
    for (int k = 0; k < 3; k++) { const float half = 0.5f * (bmax[k] - bmin[k]) / (float) res[k]; lo[k] = bmin[k] + half; hi[k] = bmax[k] - half; }
    merhost::writeVol(path, v.data(), res[0], res[1], res[2], 3, lo, hi);
}

int main(int argc, char **argv) {
    std::map<std::string, std::string> defines;
    std::string out = "out.npy", scenePath;
    int spp = 0, device = 0, layout = MER_LAYOUT_AUTO; unsigned long long seed = 0; bool raw = false;
    bool ordered = false;          // --ordered: one render per sample index, films added in index order
    int meshSdf = -1;              // --mesh-sdf[=N]: -1 off, 0 = the rif volume's grid, N = nodes on the longest axis of the mesh's box
    int fluenceRes[3] = {0, 0, 0}; bool fluence = false, multi = false;   // --fluence=NX,NY,NZ: the fluence grid of a ptracer scene instead of its film
    bool timeResolved = false;     // --time-resolved: that grid per frame of the film's transient window
    bool trackLength = false;      // --track-length: that grid from the track-length estimator (mer_fluence_track_create)
    int exitanceRes[2] = {0, 0}; bool exitance = false;                   // --exitance=NU,NV: the exitance map over the medium shape's boundary instead of the film
    std::vector<double> frequencies; bool frequencyDomain = false;        // --frequencies=K1[,K2,...]: the frequency-domain form of --fluence / --exitance
    float acceptCos = 0.0f; bool acceptCosSet = false;                    // --accept-cos=C: the acceptance cone of that map
    int sensitivityRes[3] = {0, 0, 0}; bool sensitivity = false;          // --sensitivity=NX,NY,NZ: the sensitivity grid of a detector on the boundary instead of the film
    mer_detector_desc detector; std::memset(&detector, 0, sizeof(detector)); bool detectorSet = false, gateSet = false;   // --detector=..., --gate=TMIN,TBIN
    int detectorBins[2] = {0, 0}, gates = 1; bool binsSet = false, gatesSet = false, scatter = false;   // --detector-bins=BU,BV, --gates=N, --scatter: the array form
    std::vector<int> devices; int shardMode = MER_SHARD_SAMPLES;          // several GPUs (the reference: -p <workers>, src/mitsuba/mitsuba.cpp:281)
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "-D" && i + 1 < argc) { std::string kv = argv[++i]; size_t q = kv.find('='); if (q == std::string::npos) { std::fprintf(stderr, "-D expects key=value\n"); return 2; } defines[kv.substr(0, q)] = kv.substr(q + 1); }
        else if (a.rfind("-D", 0) == 0 && a.size() > 2) { std::string kv = a.substr(2); size_t q = kv.find('='); if (q != std::string::npos) defines[kv.substr(0, q)] = kv.substr(q + 1); }
        else if (a == "-o" && i + 1 < argc) out = argv[++i];
        else if (a == "-s" && i + 1 < argc) spp = std::atoi(argv[++i]);
        else if (a == "--seed" && i + 1 < argc) seed = std::strtoull(argv[++i], NULL, 10);
        else if (a == "--device" && i + 1 < argc) device = std::atoi(argv[++i]);
        else if (a == "--gpus" && i + 1 < argc) { multi = true; const int n = std::atoi(argv[++i]); if (n < 1) { std::fprintf(stderr, "--gpus expects a positive count\n"); return 2; } devices.clear(); for (int k = 0; k < n; k++) devices.push_back(k); }
        else if (a == "--devices" && i + 1 < argc) { multi = true; devices.clear(); const std::string l = argv[++i]; size_t p = 0; while (p <= l.size()) { size_t e = l.find(',', p); if (e == std::string::npos) e = l.size(); if (e > p) devices.push_back(std::atoi(l.substr(p, e - p).c_str())); p = e + 1; } }
        else if (a == "--tiles") shardMode = MER_SHARD_TILES;
        else if (a == "--dense") layout = MER_LAYOUT_DENSE;
        else if (a == "--cell8") layout = MER_LAYOUT_CELL8;
        else if (a == "--raw") raw = true;
        else if (a == "--ordered") ordered = true;
        else if (a == "--mesh-sdf") meshSdf = 0;
        else if (a.rfind("--mesh-sdf=", 0) == 0) {
            char *e = NULL; const long n = std::strtol(a.c_str() + 11, &e, 10);
            if (e == a.c_str() + 11 || *e || n < 2 || n > 4096) { std::fprintf(stderr, "--mesh-sdf=N expects a node count between 2 and 4096\n"); return 2; }
            meshSdf = (int) n;
        }
        else if (a == "--fluence" || a.rfind("--fluence=", 0) == 0) {
            if (a.size() < 10 || !merhost::parseFluenceRes(a.substr(10), fluenceRes)) { std::fprintf(stderr, "--fluence=NX,NY,NZ expects three cell counts between 1 and 1024 (at most 2^27 cells)\n"); return 2; }
            fluence = true;
        }
        else if (a == "--exitance" || a.rfind("--exitance=", 0) == 0) {
            if (a.size() < 11 || !merhost::parseExitanceRes(a.substr(11), exitanceRes)) { std::fprintf(stderr, "--exitance=NU,NV expects two cell counts between 1 and 4096\n"); return 2; }
            exitance = true;
        }
        else if (a == "--sensitivity" || a.rfind("--sensitivity=", 0) == 0) {
            if (a.size() < 14 || !merhost::parseFluenceRes(a.substr(14), sensitivityRes)) { std::fprintf(stderr, "--sensitivity=NX,NY,NZ expects three cell counts between 1 and 1024 (at most 2^27 cells)\n"); return 2; }
            sensitivity = true;
        }
        else if (a.rfind("--detector=", 0) == 0) {
            if (!merhost::parseDetector(a.substr(11), detector)) { std::fprintf(stderr, "--detector=FACE,NU,NV,IU0,IU1,IV0,IV1 expects a face 0 ... 5, two cell counts between 1 and 4096 and a window 0 <= IU0 < IU1 <= NU, 0 <= IV0 < IV1 <= NV\n"); return 2; }
            detectorSet = true;
        }
        else if (a.rfind("--gate=", 0) == 0) {
            char *e = NULL, *e2 = NULL; detector.t_min = std::strtof(a.c_str() + 7, &e);
            if (e != a.c_str() + 7 && *e == ',') detector.t_bin = std::strtof(e + 1, &e2);
            if (!e2 || e2 == e + 1 || *e2 || !std::isfinite(detector.t_min) || !std::isfinite(detector.t_bin) || !(detector.t_bin > 0.0f)) { std::fprintf(stderr, "--gate=TMIN,TBIN expects a finite start and a width greater than 0, in optical path length\n"); return 2; }
            gateSet = true;
        }
        else if (a.rfind("--detector-bins=", 0) == 0) {
            if (!merhost::parseExitanceRes(a.substr(16), detectorBins)) { std::fprintf(stderr, "--detector-bins=BU,BV expects two cell counts between 1 and 4096\n"); return 2; }
            binsSet = true;
        }
        else if (a.rfind("--gates=", 0) == 0) {
            char *e = NULL; const long n = std::strtol(a.c_str() + 8, &e, 10);
            if (e == a.c_str() + 8 || *e || n < 1 || n > (1L << 27)) { std::fprintf(stderr, "--gates=N expects a count of at least 1\n"); return 2; }
            gates = (int) n; gatesSet = true;
        }
        else if (a == "--scatter") scatter = true;
        else if (a.rfind("--accept-cos=", 0) == 0) {
            char *e = NULL; acceptCos = std::strtof(a.c_str() + 13, &e);
            if (e == a.c_str() + 13 || *e || !(acceptCos >= 0.0f && acceptCos < 1.0f)) { std::fprintf(stderr, "--accept-cos=C expects a cosine with 0 <= C < 1\n"); return 2; }
            acceptCosSet = true;
        }
        else if (a == "--frequencies" || a.rfind("--frequencies=", 0) == 0) {
            const int bad = a.size() < 14 ? 1 : merhost::parseFrequencies(a.substr(14), frequencies);
            if (bad == 1) { std::fprintf(stderr, "--frequencies=K1[,K2,...] expects a comma-separated list of wavenumbers (radians per unit of optical path length)\n"); return 2; }
            if (bad == 2) { std::fprintf(stderr, "--frequencies takes at most 8 wavenumbers\n"); return 2; }
            if (bad == 3) { std::fprintf(stderr, "--frequencies: a wavenumber must be finite and at least 0\n"); return 2; }
            frequencyDomain = true;
        }
        else if (a == "--time-resolved") timeResolved = true;
        else if (a == "--track-length") trackLength = true;
        else if (a == "-h" || a == "--help") { std::printf("usage: mer_render [-D key=value]... [-s spp] [-o out.npy|out.pfm|out.exr] [--raw] [--dense|--cell8] [--device n | --gpus N | --devices a,b,...] [--tiles] [--mesh-sdf[=N]] [--ordered] [--fluence=NX,NY,NZ [--time-resolved | --track-length]] [--exitance=NU,NV [--time-resolved] [--accept-cos=C]] [--frequencies=K1[,K2,...]] [--sensitivity=NX,NY,NZ --detector=FACE,NU,NV,IU0,IU1,IV0,IV1 [--accept-cos=C] [--gate=TMIN,TBIN] [--detector-bins=BU,BV] [--gates=N] [--scatter]] scene.xml\n"
                                                         "  --mesh-sdf[=N]: a heterogeneousrefractive medium in an obj shape without an sdf child: build the signed-distance grid of the faces on the GPU\n"
                                                         "  and render with it as the boundary; grid = the rif volume's box and resolution, or with N the mesh's box + 5 %% with N nodes on its longest axis\n"
                                                         "  --ordered: one render per sample index, the films added in index order: the film does not depend on the order of its float atomics across\n"
                                                         "  samples (bit-reproducible when every sample lands in one pixel: box filter of radius 0.5); slower\n"
                                                         "  --gpus N / --devices: one context per listed GPU, volumes replicated, samples (default) or 32x32 image tiles (--tiles) sharded over them,\n"
                                                         "  films reduced with RCCL (distinct devices) or peer copies (a device listed twice)\n"
                                                         "  --fluence=NX,NY,NZ: a `ptracer` scene: instead of the film, the fluence inside the medium on a grid of NX x NY x NZ cells over the medium\n"
                                                         "  shape's bounding box, from width x height x spp light paths on one GPU; -o names a 3-channel float32 VOL (version 3) whose box is that of\n"
                                                         "  the cell centres, so that a gridvolume reading it interpolates between them; the totals are printed\n"
                                                         "  --time-resolved (with --fluence=): the scene's film must have decomposition = transient; every deposit is also binned by its optical path\n"
                                                         "  length into the film's window (minBound, binWidth, ceil((maxBound - minBound) / binWidth) frames); -o names a float32 .npy\n"
                                                         "  [frames][nz][ny][nx][3] = sums / (paths x cell volume x binWidth); the totals also print the weight outside the window\n"
                                                         "  --track-length (with --fluence=, not with --time-resolved): the track-length estimator: every free flight deposits along its path, cut at\n"
                                                         "  the cell faces, so that cells without extinction hold their fluence too; the distance sampling must be analog (a gridded sigma_t, or a\n"
                                                         "  homogeneous one with mediumSamplingWeight 1 and strategy single / manual, or balance with equal sigma_t); `dropped` is weight x length\n"
                                                         "  --exitance=NU,NV: a `ptracer` scene: instead of the film, where the light paths leave the medium: NU x NV cells on every face of the medium\n"
                                                         "  shape's boundary (cube: 6 faces, sphere: 1 face of equal-area cells), from width x height x spp light paths on one GPU; -o names a float32\n"
                                                         "  .npy [frames][faces][nv][nu][3] = sums / (paths x cell area [x binWidth]); the 16 totals are printed.  --time-resolved takes the window\n"
                                                         "  from the film as for --fluence; --accept-cos=C bins only the exits within the cone cos >= C about the outward normal\n"
                                                         "  --frequencies=K1[,K2,...] (with --fluence= or --exitance=; not with --time-resolved, --track-length): the frequency-domain form, the response\n"
                                                         "  to an intensity-modulated source: up to 8 wavenumbers k = 2 pi f / c0 >= 0 in radians per unit of optical path length (0: the steady state);\n"
                                                         "  every deposit goes as w (cos, sin)(k l) into a real and an imaginary plane per wavenumber.  -o names a float32 .npy\n"
                                                         "  [n_freq][2][nz][ny][nx][3] = sums / (paths x cell volume) or [n_freq][2][faces][nv][nu][3] = sums / (paths x cell area); the totals and, per\n"
                                                         "  wavenumber, the amplitude and phase of the summed planes are printed.  --accept-cos=C works with the map\n"
                                                         "  --sensitivity=NX,NY,NZ --detector=FACE,NU,NV,IU0,IU1,IV0,IV1: a `ptracer` scene: instead of the film, which part of the medium the light\n"
                                                         "  that reached a detector travelled through (the absorption Jacobian).  The detector is the cell window IU0 <= iu < IU1, IV0 <= iv < IV1 on\n"
                                                         "  face FACE of an --exitance raster of NU x NV cells; --accept-cos=C narrows it to a cone, --gate=TMIN,TBIN to the optical path lengths\n"
                                                         "  TMIN <= l < TMIN + TBIN.  The detected paths are walked a second time and deposit weight x length on a grid of NX x NY x NZ cells over\n"
                                                         "  the medium shape's bounding box; -o names a 3-channel float32 VOL of J / paths (minus the derivative of the detected signal per path by\n"
                                                         "  a cell's sigma_a), laid out as --fluence lays its VOL out; the totals are printed.  One GPU; not with --fluence, --exitance, --gpus or --devices\n"
                                                         "  --detector-bins=BU,BV, --gates=N, --scatter (with --sensitivity= and --detector=): an array of detectors in one render.  One detector is\n"
                                                         "  BU x BV raster cells of the window (BU, BV must divide it; default: the whole window), gate g takes TMIN + g TBIN <= l < TMIN + (g + 1) TBIN\n"
                                                         "  for g < N (N > 1 needs --gate=), --scatter adds the scattering grids K (the detected weight per scattering collision in a cell; with a\n"
                                                         "  homogeneous sigma_s the derivative of a detector's signal by sigma_s is K / sigma_s - J).  -o names a float32 .npy\n"
                                                         "  [1 + scatter][gates][ndv][ndu][nz][ny][nx][3] = sums / paths; one line per measurement is printed: gate, dv, du, detected paths and weight\n"); return 0; }
        else scenePath = a;
    }
    if (frequencyDomain) {
        if (sensitivity) { std::fprintf(stderr, "--frequencies belongs to --fluence / --exitance: a frequency-domain sensitivity grid is not built\n"); return 2; }
        if (!fluence && !exitance) { std::fprintf(stderr, "--frequencies needs --fluence=NX,NY,NZ or --exitance=NU,NV\n"); return 2; }
        if (timeResolved) { std::fprintf(stderr, "--frequencies and --time-resolved exclude each other: the frequency-domain form has no window\n"); return 2; }
        if (trackLength) { std::fprintf(stderr, "--frequencies and --track-length exclude each other: a frequency-domain track-length grid is not built\n"); return 2; }
        if (multi) { std::fprintf(stderr, "--frequencies runs on one GPU (--device): --gpus / --devices are not built for it (raw sums of shards add; the reduction is left to the caller)\n"); return 2; }
        if (fluence && !exitance) {
            if (out == "out.npy") out = "fluence_fd.npy";
            if (!(out.size() > 4 && out.substr(out.size() - 4) == ".npy")) { std::fprintf(stderr, "--frequencies writes a .npy file ([n_freq][2][nz][ny][nx][3]): a VOL holds 1 or 3 channels\n"); return 2; }
        }
    }
    if (exitance && fluence) { std::fprintf(stderr, "--exitance and --fluence exclude each other: one map per run\n"); return 2; }
    if (exitance && multi) { std::fprintf(stderr, "--exitance runs on one GPU (--device): --gpus / --devices are not built for it (raw sums of shards add; the reduction is left to the caller)\n"); return 2; }
    if (exitance && trackLength) { std::fprintf(stderr, "--track-length belongs to --fluence=NX,NY,NZ: an exitance map has no track-length form\n"); return 2; }
    if (sensitivity && (fluence || exitance)) { std::fprintf(stderr, "--sensitivity excludes --fluence and --exitance: one map per run\n"); return 2; }
    if (sensitivity && multi) { std::fprintf(stderr, "--sensitivity runs on one GPU (--device): --gpus / --devices are not built for it (raw sums of shards add; the reduction is left to the caller)\n"); return 2; }
    if (sensitivity && (timeResolved || trackLength)) { std::fprintf(stderr, "--time-resolved and --track-length belong to --fluence / --exitance: a sensitivity grid has the one gate of --gate=TMIN,TBIN\n"); return 2; }
    if (sensitivity && !detectorSet) { std::fprintf(stderr, "--sensitivity needs --detector=FACE,NU,NV,IU0,IU1,IV0,IV1\n"); return 2; }
    if ((detectorSet || gateSet) && !sensitivity) { std::fprintf(stderr, "--detector and --gate need --sensitivity=NX,NY,NZ\n"); return 2; }
    const bool array = binsSet || gatesSet || scatter;
    if (array && !(sensitivity && detectorSet)) { std::fprintf(stderr, "--detector-bins, --gates and --scatter need --sensitivity=NX,NY,NZ and --detector=FACE,NU,NV,IU0,IU1,IV0,IV1\n"); return 2; }
    if (gates > 1 && !gateSet) { std::fprintf(stderr, "--gates=N above 1 needs --gate=TMIN,TBIN: the first gate and the width of every gate\n"); return 2; }
    if (binsSet && ((detector.iu1 - detector.iu0) % detectorBins[0] || (detector.iv1 - detector.iv0) % detectorBins[1])) { std::fprintf(stderr, "--detector-bins=BU,BV must divide the window of --detector (IU1 - IU0 and IV1 - IV0)\n"); return 2; }
    if (array) {
        if (out == "out.npy") out = "sensitivity.npy";
        if (!(out.size() > 4 && out.substr(out.size() - 4) == ".npy")) { std::fprintf(stderr, "--detector-bins, --gates and --scatter write a .npy file ([1 + scatter][gates][ndv][ndu][nz][ny][nx][3])\n"); return 2; }
    }
    if (acceptCosSet && !exitance && !sensitivity) { std::fprintf(stderr, "--accept-cos needs --exitance=NU,NV\n"); return 2; }
    if (exitance) {
        if (out == "out.npy") out = "exitance.npy";
        if (!(out.size() > 4 && out.substr(out.size() - 4) == ".npy")) { std::fprintf(stderr, "--exitance writes a .npy file ([frames][faces][nv][nu][3])\n"); return 2; }
    }
    if (fluence && multi) { std::fprintf(stderr, "--fluence runs on one GPU (--device): --gpus / --devices are not built for it (raw sums of shards add; the reduction is left to the caller)\n"); return 2; }
    if (timeResolved && !fluence && !exitance) { std::fprintf(stderr, "--time-resolved needs --fluence=NX,NY,NZ\n"); return 2; }
    if (trackLength && !fluence) { std::fprintf(stderr, "--track-length needs --fluence=NX,NY,NZ\n"); return 2; }
    if (trackLength && timeResolved) { std::fprintf(stderr, "--track-length and --time-resolved exclude each other: a time-resolved track-length grid does not exist\n"); return 2; }
    if (timeResolved && !exitance) {
        if (out == "out.npy") out = "fluence_t.npy";
        if (!(out.size() > 4 && out.substr(out.size() - 4) == ".npy")) { std::fprintf(stderr, "--time-resolved writes a .npy file ([frames][nz][ny][nx][3]): a VOL holds 1 or 3 channels\n"); return 2; }
    }
    if (scenePath.empty()) { std::fprintf(stderr, "mer_render: no scene file given\n"); return 2; }
    try {
        auto scene = merhost::loadScene(scenePath, defines);
        const auto printPlanes = [&](const std::vector<double> &sums, size_t perPlane) {      // per wavenumber: the planes summed over cells and channels
            for (size_t j = 0; j < frequencies.size(); j++) {
                double re = 0.0, im = 0.0;
                for (size_t i = 0; i < perPlane; i++) { re += sums[(2 * j) * perPlane + i]; im += sums[(2 * j + 1) * perPlane + i]; }
                std::printf("frequency %zu  k %.9g  amplitude %.9g  phase %.9g\n", j, frequencies[j], std::hypot(re, im), std::atan2(im, re));
            }
        };
        if (exitance && frequencyDomain) {
            const merhost::Integrator::Exitance x = scene->integrator->renderExitance(*scene, device, exitanceRes, frequencies, acceptCos, spp, seed);
            const std::vector<float> m = x.exitance();
            merhost::writeNpy(out, m.data(), std::vector<int>{(int) frequencies.size(), 2, x.faces, x.resV, x.resU, 3});
            std::printf("paths %.0f  escaped %.9g %.9g %.9g  missed %.9g %.9g %.9g  ended %.0f  late %.9g %.9g %.9g  rejected %.9g %.9g %.9g  binned %.0f  %.0f\n",
                        x.totals[0], x.totals[1], x.totals[2], x.totals[3], x.totals[4], x.totals[5], x.totals[6], x.totals[7], x.totals[8], x.totals[9], x.totals[10],
                        x.totals[11], x.totals[12], x.totals[13], x.totals[14], x.totals[15]);
            printPlanes(x.sums, (size_t) x.faces * x.resV * x.resU * 3);
            std::printf("wrote %s (%zu frequencies of %d faces of %dx%d cells)\n", out.c_str(), frequencies.size(), x.faces, x.resU, x.resV);
            return 0;
        }
        if (fluence && frequencyDomain) {
            const merhost::Integrator::Fluence f = scene->integrator->renderFluence(*scene, device, fluenceRes, frequencies, spp, seed);
            const std::vector<float> phi = f.phi();
            merhost::writeNpy(out, phi.data(), std::vector<int>{(int) frequencies.size(), 2, f.res[2], f.res[1], f.res[0], 3});
            std::printf("paths %.0f  escaped %.9g %.9g %.9g  dropped %.9g %.9g %.9g  ended %.0f\n", f.totals[0], f.totals[1], f.totals[2], f.totals[3],
                        f.totals[4], f.totals[5], f.totals[6], f.totals[7]);
            printPlanes(f.sums, (size_t) f.res[0] * f.res[1] * f.res[2] * 3);
            std::printf("wrote %s (%zu frequencies of %dx%dx%d cells)\n", out.c_str(), frequencies.size(), f.res[0], f.res[1], f.res[2]);
            return 0;
        }
        if (exitance) {
            const Window w = timeResolved ? filmWindow(*scene) : Window{1, 0.0f, 0.0f};
            const merhost::Integrator::Exitance x = scene->integrator->renderExitance(*scene, device, exitanceRes, w.frames, w.tMin, w.tBin, acceptCos, spp, seed);
            const std::vector<float> m = x.exitance();
            merhost::writeNpy(out, m.data(), std::vector<int>{x.frames, x.faces, x.resV, x.resU, 3});
            std::printf("paths %.0f  escaped %.9g %.9g %.9g  missed %.9g %.9g %.9g  ended %.0f  late %.9g %.9g %.9g  rejected %.9g %.9g %.9g  binned %.0f  %.0f\n",
                        x.totals[0], x.totals[1], x.totals[2], x.totals[3], x.totals[4], x.totals[5], x.totals[6], x.totals[7], x.totals[8], x.totals[9], x.totals[10],
                        x.totals[11], x.totals[12], x.totals[13], x.totals[14], x.totals[15]);
            std::printf("wrote %s (%d frames of %d faces of %dx%d cells)\n", out.c_str(), x.frames, x.faces, x.resU, x.resV);
            return 0;
        }
        if (sensitivity && array) {
            detector.cos_min = acceptCos;
            const merhost::Integrator::SensitivityArray j = scene->integrator->renderSensitivityArray(
                *scene, device, sensitivityRes, detector, binsSet ? detectorBins[0] : detector.iu1 - detector.iu0, binsSet ? detectorBins[1] : detector.iv1 - detector.iv0, gates, scatter, spp, seed);
            const std::vector<float> v = j.jacobian();
            merhost::writeNpy(out, v.data(), std::vector<int>{1 + j.scatter, j.gates, j.ndv, j.ndu, j.res[2], j.res[1], j.res[0], 3});
            std::printf("paths %.0f  detected weight %.9g %.9g %.9g  dropped %.9g %.9g %.9g  ended %.0f  detected %.0f  weight x length %.9g %.9g %.9g  disagreements %.0f  collisions dropped %.9g %.9g %.9g\n",
                        j.totals[0], j.totals[1], j.totals[2], j.totals[3], j.totals[4], j.totals[5], j.totals[6], j.totals[7], j.totals[8], j.totals[9], j.totals[10],
                        j.totals[11], j.totals[12], j.totals[13], j.totals[14], j.totals[15]);
            for (int g = 0; g < j.gates; g++)
                for (int dv = 0; dv < j.ndv; dv++)
                    for (int du = 0; du < j.ndu; du++) {
                        const double *m = &j.meas[(((size_t) g * j.ndv + dv) * j.ndu + du) * 8];
                        std::printf("measurement gate %d dv %d du %d  detected %.0f  weight %.9g %.9g %.9g\n", g, dv, du, m[3], m[0], m[1], m[2]);
                    }
            std::printf("wrote %s (%d x %d x %d x %d grids of %dx%dx%d cells)\n", out.c_str(), 1 + j.scatter, j.gates, j.ndv, j.ndu, j.res[0], j.res[1], j.res[2]);
            return 0;
        }
        if (sensitivity) {
            if (out == "out.npy") out = "sensitivity.vol";
            detector.cos_min = acceptCos;
            const merhost::Integrator::Sensitivity j = scene->integrator->renderSensitivity(*scene, device, sensitivityRes, detector, spp, seed);
            const std::vector<float> v = j.jacobian();
            writeCellVol(out, v, j.res, j.bmin, j.bmax);
            std::printf("paths %.0f  detected weight %.9g %.9g %.9g  dropped %.9g %.9g %.9g  ended %.0f  detected %.0f  weight x length %.9g %.9g %.9g  disagreements %.0f\n",
                        j.totals[0], j.totals[1], j.totals[2], j.totals[3], j.totals[4], j.totals[5], j.totals[6], j.totals[7], j.totals[8], j.totals[9], j.totals[10],
                        j.totals[11], j.totals[12]);
            std::printf("wrote %s (%dx%dx%d cells)\n", out.c_str(), j.res[0], j.res[1], j.res[2]);
            return 0;
        }
        if (fluence && timeResolved) {
            const Window w = filmWindow(*scene);
            const merhost::Integrator::Fluence f = scene->integrator->renderFluence(*scene, device, fluenceRes, w.frames, w.tMin, w.tBin, spp, seed);
            const std::vector<float> phi = f.phi();
            merhost::writeNpy(out, phi.data(), std::vector<int>{f.frames, f.res[2], f.res[1], f.res[0], 3});
            std::printf("paths %.0f  escaped %.9g %.9g %.9g  dropped %.9g %.9g %.9g  ended %.0f  out of window %.9g %.9g %.9g\n", f.totals[0], f.totals[1], f.totals[2],
                        f.totals[3], f.totals[4], f.totals[5], f.totals[6], f.totals[7], f.totals[8], f.totals[9], f.totals[10]);
            std::printf("wrote %s (%d frames of %dx%dx%d cells)\n", out.c_str(), f.frames, f.res[0], f.res[1], f.res[2]);
            return 0;
        }
        if (fluence) {
            if (out == "out.npy") out = "fluence.vol";
            const merhost::Integrator::Fluence f = scene->integrator->renderFluence(*scene, device, fluenceRes, spp, seed, trackLength);
            const std::vector<float> phi = f.phi();
            writeCellVol(out, phi, f.res, f.bmin, f.bmax);
            std::printf("paths %.0f  escaped %.9g %.9g %.9g  dropped %.9g %.9g %.9g  ended %.0f\n", f.totals[0], f.totals[1], f.totals[2], f.totals[3],
                        f.totals[4], f.totals[5], f.totals[6], f.totals[7]);
            std::printf("wrote %s (%dx%dx%d cells)\n", out.c_str(), f.res[0], f.res[1], f.res[2]);
            return 0;
        }
        const int w = scene->sensor->film->width, h = scene->sensor->film->height;
        if (devices.empty()) devices.push_back(device);
        std::vector<float> film = scene->integrator->render(*scene, devices, shardMode, spp, seed, layout, meshSdf, ordered);
        const int frames = scene->sensor->film->frames();
        if (raw) merhost::writeNpy(out, film.data(), h, w, frames * 3 + 2);
        else {
            std::vector<float> rgb = merhost::develop(film, w, h, frames);
            const bool pfm = out.size() > 4 && out.substr(out.size() - 4) == ".pfm";
            const bool exr = out.size() > 4 && out.substr(out.size() - 4) == ".exr";
            if (frames == 1) { if (pfm) merhost::writePfm(out, rgb.data(), h, w); else if (exr) merhost::writeExr(out, rgb.data(), h, w); else merhost::writeNpy(out, rgb.data(), h, w, 3); }
            else if (exr) {
                for (int f = 0; f < frames; f++) {
                    char suffix[32]; std::snprintf(suffix, sizeof(suffix), "_%04d.exr", f);
                    merhost::writeExr(out.substr(0, out.size() - 4) + suffix, rgb.data() + (size_t) f * w * h * 3, h, w);
                }
            }
            else if (pfm) {                       // one file per frame, as the reference's hdrfilm writes <name>_<frame>
                for (int f = 0; f < frames; f++) {
                    char suffix[32]; std::snprintf(suffix, sizeof(suffix), "_%04d.pfm", f);
                    merhost::writePfm(out.substr(0, out.size() - 4) + suffix, rgb.data() + (size_t) f * w * h * 3, h, w);
                }
            } else merhost::writeNpy(out, rgb.data(), frames * h, w, 3);     // [frames*h][w][3]
        }
        std::printf("wrote %s (%dx%d)\n", out.c_str(), w, h);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "mer_render: %s\n", e.what());      // reference: the worker catches std::runtime_error and cancels
        return 1;
    }
    return 0;
}
