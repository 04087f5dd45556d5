// mer_host.h -- C++ host side above the C-ABI (include/mer.h): a mirror of the reference's plugin interface for
// the hot path.  Same plugin type names, parameter names, defaults and error texts as cmu-ci-lab/MitsubaER
// (SURVEY.md section 9.1), none of its machinery (no Boost, Xerces, ref-counting, serialization, scheduler).
//
//   Properties            include/mitsuba/core/properties.h:46
//   ConfigurableObject    addChild(name, child) / configure()        src/librender/scenehandler.cpp:712-777
//   VolumeDataSource      gridvolume | splinevolume | constvolume    include/mitsuba/render/volume.h:32-109
//   PhaseFunction         hg | isotropic                             include/mitsuba/render/phase.h:117-241
//   Medium                homogeneous | heterogeneous | heterogeneousrefractive   include/mitsuba/render/medium.h:113-234
//   Shape                 cube | sphere | obj (bounding box), `interior` medium, null BSDF   src/librender/shape.cpp:48-70,166-190
//   Sensor / Film / ReconstructionFilter / Sampler      perspective | orthographic | thinlens | telecentric, hdrfilm, gaussian | box, independent | ldsampler
//   Emitter               constant | point | area (on a rectangle shape) | collimated (ptracer)
//   Integrator            volpath | ptracer -> render() flattens the scene to mer_scene_desc and calls mer_render
//   SceneHandler          scene-XML subset with $param substitution    src/librender/scenehandler.cpp, src/mitsuba/mitsuba.cpp:58,168-173
//
// Errors: like Log(EError) in the reference (src/libcore/logger.cpp:100-147) every failure throws std::runtime_error.
#pragma once
#include <cmath>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/mer.h"

namespace merhost {

struct Spectrum { float c[3]; };
struct Vec3 { float x, y, z; };

[[noreturn]] void Log_EError(const std::string &msg);      // throws std::runtime_error(msg)

// ---------------------------------------------------------------------------------------------------------------
class Properties {
public:
    enum Type { EBoolean, EInteger, EFloat, EString, ESpectrum, EPoint, ETransform };
    explicit Properties(const std::string &pluginName = "") : m_pluginName(pluginName) {}
    const std::string &getPluginName() const { return m_pluginName; }
    const std::string &getID() const { return m_id; }
    void setID(const std::string &id) { m_id = id; }
    bool hasProperty(const std::string &name) const { return m_entries.count(name) != 0; }
    Type getType(const std::string &name) const;
    void setBoolean(const std::string &n, bool v);
    void setInteger(const std::string &n, int v);
    void setFloat(const std::string &n, float v);
    void setString(const std::string &n, const std::string &v);
    void setSpectrum(const std::string &n, const Spectrum &v);
    void setPoint(const std::string &n, const Vec3 &v);
    void setTransform(const std::string &n, const float m[16]);
    bool getBoolean(const std::string &n) const;
    bool getBoolean(const std::string &n, bool def) const;
    int getInteger(const std::string &n) const;
    int getInteger(const std::string &n, int def) const;
    float getFloat(const std::string &n) const;
    float getFloat(const std::string &n, float def) const;
    std::string getString(const std::string &n) const;
    std::string getString(const std::string &n, const std::string &def) const;
    Spectrum getSpectrum(const std::string &n) const;
    Spectrum getSpectrum(const std::string &n, const Spectrum &def) const;
    Vec3 getPoint(const std::string &n) const;
    Vec3 getPoint(const std::string &n, const Vec3 &def) const;
    void getTransform(const std::string &n, float m[16]) const;      // identity when absent
    /// names never queried by the plugin: the reference warns about them (properties.cpp getUnqueried)
    std::vector<std::string> getUnqueried() const;
private:
    struct Entry { Type type; bool b = false; int i = 0; float f = 0; std::string s; Spectrum spec{}; Vec3 p{}; float m[16]; mutable bool queried = false; };
    const Entry &get(const std::string &n, Type t) const;
    std::string m_pluginName, m_id;
    std::map<std::string, Entry> m_entries;
};

// ---------------------------------------------------------------------------------------------------------------
class ConfigurableObject {
public:
    virtual ~ConfigurableObject() {}
    virtual const char *getClassName() const = 0;           // MTS_CLASS analogue: "Medium", "VolumeDataSource", ...
    virtual void addChild(const std::string &name, std::shared_ptr<ConfigurableObject> child);
    virtual void configure() {}
    virtual std::string toString() const { return getClassName(); }
};
typedef std::shared_ptr<ConfigurableObject> ObjRef;

class VolumeDataSource : public ConfigurableObject {
public:
    const char *getClassName() const override { return "VolumeDataSource"; }
    virtual bool supportsFloatLookups() const { return false; }
    virtual bool supportsSpectrumLookups() const { return false; }
    virtual bool isConstant() const { return false; }
    virtual bool isSpline() const { return false; }
    virtual bool isAcoustic() const { return false; }           // acousticrifvolume: analytic, no payload
    float ac_n_o = 1.3333f, ac_n_max = 0.0f, ac_k_r = 0.0f; int ac_mode = 0;
    float aabb_min[3] = {0, 0, 0}, aabb_max[3] = {0, 0, 0};
    float worldToVolume[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // inverse of `toWorld`, row-major 3x4; all zeros = identity (gridvolume.cpp:110,188-189)
    int res[3] = {0, 0, 0}, channels = 0, dtype = MER_VOL_F32;
    std::vector<unsigned char> data;          // dense payload (gridvolume / splinevolume)
    Spectrum constant{};                      // constvolume
    std::string filename;
    float getStepSize() const;                // gridvolume.cpp:196-198
    float getMaximumFloatValue() const { return 1.0f; }     // gridvolume.cpp:583-585
};

class PhaseFunction : public ConfigurableObject {
public:
    const char *getClassName() const override { return "PhaseFunction"; }
    int kind = MER_PHASE_ISOTROPIC; float g = 0.0f;
    float getMeanCosine() const { return kind == MER_PHASE_HG ? g : 0.0f; }
};

class Medium : public ConfigurableObject {
public:
    const char *getClassName() const override { return "Medium"; }
    void addChild(const std::string &name, ObjRef child) override;
    void configure() override;
    virtual bool isHomogeneous() const { return kind == "homogeneous"; }
    bool isheterogeneousrefractive() const { return kind == "heterogeneousrefractive"; }
    std::string kind;                          // plugin name
    Spectrum sigmaA{}, sigmaS{};               // homogeneous coefficients after `scale`
    int strategy = MER_STRATEGY_BALANCE, channel = -1; float samplingDensity = 0, mediumSamplingWeight = -1;
    float scale = 1.0f;                        // heterogeneous `scale`
    float stepsize = 1e-3f;                    // heterogeneousrefractive `stepsize`
    bool aggressiveTracing = false;            // heterogeneousrefractive `aggressivetracing` (needs the `sdf` child)
    int stepper = MER_STEP_VERLET, trEstimator = MER_TR_WOODCOCK2;
    int method = MER_METHOD_WOODCOCK; float hetStepSize = 0;       ///< heterogeneous `method`, `stepSize` (heterogeneous.cpp:183-202)
    Spectrum emission{};
    std::shared_ptr<VolumeDataSource> density, albedo, rif, sdf;
    std::shared_ptr<PhaseFunction> phase;
};

class Shape : public ConfigurableObject {
public:
    const char *getClassName() const override { return "Shape"; }
    void addChild(const std::string &name, ObjRef child) override;
    int boundary = MER_BOUNDARY_AABB;
    float bmin[3] = {-1, -1, -1}, bmax[3] = {1, 1, 1}, center[3] = {0, 0, 0}, radius = 1;
    std::shared_ptr<Medium> interior;
    /// `obj`: the faces next to the bounding box, toWorld applied to the vertices (xyz per vertex; 3 vertex indices per triangle, polygons as
    /// fans).  Reader rules of mitsubaer_amd/meshio.py.  Read by Integrator::meshSdfGrid / render(..., meshSdf) only
    bool isObj = false; std::vector<float> meshVertices; std::vector<int32_t> meshTriangles;
    std::string meshError;             ///< a face record that could not be read (the faces stop there): raised by meshSdfGrid, which alone uses them
    bool isRectangle = false; float rectToWorld[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};   ///< `rectangle` (src/shapes/rectangle.cpp): carrier of an area emitter
    /// the emitter-list entry type this shape yields with an `area` emitter child: MER_EMITTER_AREA (`rectangle`), MER_EMITTER_AREA_DISK
    /// (`disk`, src/shapes/disk.cpp) or MER_EMITTER_AREA_SPHERE (`sphere`, src/shapes/sphere.cpp); 0 = the shape cannot carry one.
    /// rectToWorld then is the entry's to_world (a sphere's: translate(centre) * scale(radius), z negated for flipNormals)
    int areaType = 0;
    std::string boundaryError;         ///< a `sphere` whose toWorld the medium boundary cannot take (it may still carry an emitter): raised without an emitter child
    std::shared_ptr<class Emitter> areaEmitter;
    bool hasBSDF = false;              ///< a bsdf child was given (null | hdielectric | hroughdielectric)
    int bsdf = MER_BSDF_NULL;          ///< MER_BSDF_*
    std::shared_ptr<class BSDF> bsdfObj;
};
/// BSDF of the medium shape: `null` (index-matched), `hdielectric` (src/bsdfs/hdielectric.cpp: eta = RIF at the hit point) or
/// `hroughdielectric` (src/bsdfs/hroughdielectric.cpp: its microfacet form; distribution, alpha (clamped to >= 1e-4), sampleVisible)
class BSDF : public ConfigurableObject {
public:
    const char *getClassName() const override { return "BSDF"; }
    int kind = MER_BSDF_NULL;
    int distribution = MER_MICROFACET_BECKMANN; float alpha = 0.1f; bool sampleVisible = true;
    bool isheterogeneousbsdf() const { return kind == MER_BSDF_HDIELECTRIC || kind == MER_BSDF_HROUGHDIELECTRIC; }   // hroughdielectric.cpp:59
};

class ReconstructionFilter : public ConfigurableObject {
public:
    const char *getClassName() const override { return "ReconstructionFilter"; }
    int kind = MER_FILTER_GAUSSIAN; float param = 0.5f;
};
class Sampler : public ConfigurableObject {
public:
    const char *getClassName() const override { return "Sampler"; }
    int sampleCount = 4;
};
class Film : public ConfigurableObject {
public:
    const char *getClassName() const override { return "Film"; }
    void addChild(const std::string &name, ObjRef child) override;
    int width = 768, height = 576;
    /// src/librender/film.cpp:56-84
    int decomposition = MER_DECOMPOSITION_NONE; float minBound = 0.0f, maxBound = 0.0f, binWidth = 1.0f; bool calibratedTransient = false;
    /// PathLengthSampler (src/librender/pathlengthsampler.cpp:12-40)
    int modulation = MER_MODULATION_NONE; float lambda = 1.0f, phase = 0.0f; int P = 32, neighbors = 3;
    int frames() const { return (decomposition != MER_DECOMPOSITION_NONE && modulation == MER_MODULATION_NONE) ? (int) std::ceil((maxBound - minBound) / binWidth) : 1; }
    int channels() const { return frames() * 3 + 2; }
    std::shared_ptr<ReconstructionFilter> rfilter;
};
class Sensor : public ConfigurableObject {
public:
    const char *getClassName() const override { return "Sensor"; }
    void addChild(const std::string &name, ObjRef child) override;
    float fov = 50.0f; std::string fovAxis = "x"; float nearClip = 1e-2f, farClip = 1e4f;
    int kind = MER_SENSOR_PERSPECTIVE;          // perspective | orthographic | thinlens | telecentric (src/sensors/)
    float apertureRadius = 0.0f, focusDistance = 1e4f;   // the lens kinds: world-space radius (thinlens.cpp:132, telecentric.cpp:81), `focusDistance` (sensor.cpp:162: farClip)
    float toWorld[16];
    std::shared_ptr<Film> film; std::shared_ptr<Sampler> sampler;
};
class Emitter : public ConfigurableObject {
public:
    const char *getClassName() const override { return "Emitter"; }
    enum Kind { EConstant, EPoint, EArea, ESpot, EEnvmap, ECollimated } kind = EConstant;
    Spectrum radiance{};                        // constant / area: radiance ; point / spot: intensity ; collimated: power
    Vec3 position{0, 0, 0};                     // point (src/emitters/point.cpp:60-68)
    float toWorld[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // spot: its frame (src/emitters/spot.cpp:124-131); collimated: the beam's (collimated.cpp:115-124)
    float cutoffAngle = 20, beamWidth = 15;     // spot: degrees (spot.cpp:68-73)
    float samplingWeight = 1.0f;                // `samplingWeight` (src/librender/emitter.cpp:103): selection weight among the emitters of its kind
    std::vector<float> image; int imageW = 0, imageH = 0;      // envmap: the lat-long image as loaded, float [h][w][3] (src/emitters/envmap.cpp:116-160)
    float scale = 1.0f;                         // envmap: `scale`
};

class Scene;
/// `volpath`, or `ptracer` (kind = MER_INTEGRATOR_PTRACER: light tracing, src/integrators/ptracer), executed on the GPU: Integrator::render() (include/mitsuba/render/integrator.h:74) owns its parallelism
class Integrator : public ConfigurableObject {
public:
    const char *getClassName() const override { return "Integrator"; }
    int maxDepth = -1, rrDepth = 5; bool hideEmitters = false, strictNormals = false;
    int kind = MER_INTEGRATOR_VOLPATH;          ///< MER_INTEGRATOR_*
    /// flatten (validates like the reference's configure()) -- no GPU needed.  Several point or area emitters: desc.emitters points into
    /// scene.emitterList, which must outlive desc
    /// meshGrid: the grid of a signed-distance volume that render() will build from the `obj` medium shape (meshSdfGrid): the boundary then is
    /// MER_BOUNDARY_SDF, and `aggressivetracing` takes its error bound from that grid
    void flatten(const Scene &scene, mer_scene_desc &desc, const mer_grid_desc *meshGrid = NULL) const;
    /// `mer_render --mesh-sdf[=N]`: the grid on which the signed distance of the `obj` medium shape is built (n = 0: the `rif` volume's own box and
    /// resolution; n >= 2: the mesh's bounding box grown by 5 % per side, n nodes on the longest axis, equal spacing).  Refuses, saying why, a
    /// scene that has an `sdf` child, a medium shape that is no `obj`, a medium that is not heterogeneousrefractive, a mesh the library
    /// would refuse, and n = 0 without a gridded RIF.  No GPU needed
    void meshSdfGrid(const Scene &scene, int n, mer_grid_desc &grid) const;
    /// upload volumes, render `spp` samples per pixel (0 = the sampler's sampleCount), return the film [h][w][5]
    std::vector<float> render(const Scene &scene, int device, int spp, unsigned long long seed, int layout) const;
    /// the same on several GPUs of this machine (mer_multi_*: replicated volumes, shardMode = MER_SHARD_SAMPLES | MER_SHARD_TILES, films reduced with RCCL)
    /// meshSdf: -1 = off; >= 0: build the medium shape's signed-distance grid from its faces first (meshSdfGrid(scene, meshSdf)) on the first
    /// device, download it and replicate it like any other volume.  ordered: one render per sample index, the films added on the host in index
    /// order (`mer_render --ordered`): the sum no longer depends on the order of the film's float atomics across samples
    std::vector<float> render(const Scene &scene, const std::vector<int> &devices, int shardMode, int spp, unsigned long long seed, int layout, int meshSdf = -1, bool ordered = false) const;
    /// the fluence inside the medium as a grid of res[0] x res[1] x res[2] cells over the medium shape's bounding box, recorded from the light paths
    /// of a `ptracer` scene (mer_render_fluence: the reference's `fluencemeter` + `ptracer`, a grid of probes): width x height x spp paths on
    /// one device.  Any other integrator is refused
    struct Fluence {
        int res[3]; float bmin[3], bmax[3];
        int frames = 0; float tMin = 0.0f, tBin = 0.0f;   ///< the time-resolved form: frames > 0 bins of width tBin from tMin on in optical path length
        std::vector<double> wavenumbers;        ///< the frequency-domain form: not empty, k >= 0 in radians per unit of optical path length
        std::vector<double> sums;               ///< raw sums [nz][ny][nx][3]; time-resolved: [frames][nz][ny][nx][3]; frequency-domain: [n_freq][2][nz][ny][nx][3]
        double totals[12];                      ///< paths, escaped x 3, dropped x 3, ended (mer_fluence_read); time-resolved: then out-of-window x 3 and 0 (mer_fluence_time_read)
        /// sums / (paths x cell volume), float32 [nz][ny][nx][3]; time-resolved: sums / (paths x cell volume x tBin), [frames][nz][ny][nx][3];
        /// frequency-domain: sums / (paths x cell volume), [n_freq][2][nz][ny][nx][3]
        std::vector<float> phi() const;
    };
    /// trackLength: the track-length estimator (mer_fluence_track_create): every free flight deposits along its path, voids included; the scene's
    /// distance sampling must be analog (mer.h), anything else is refused
    Fluence renderFluence(const Scene &scene, int device, const int res[3], int spp, unsigned long long seed, bool trackLength = false) const;
    /// the time-resolved form (mer_fluence_time_create): every deposit also binned by the optical path length at which it happens.  The window is
    /// the caller's; the scene's film is not read.  frames = 0: the steady-state grid.  A time-resolved track-length grid does not exist
    Fluence renderFluence(const Scene &scene, int device, const int res[3], int frames, float tMin, float tBin, int spp, unsigned long long seed, bool trackLength = false) const;
    /// the frequency-domain form (mer_fluence_fd_create): every deposit as w (cos, sin)(k l) into a real and an imaginary plane per wavenumber
    /// k (1 ... MER_MAX_FREQUENCIES of them, >= 0, radians per unit of optical path length; 0: the steady state)
    Fluence renderFluence(const Scene &scene, int device, const int res[3], const std::vector<double> &wavenumbers, int spp, unsigned long long seed) const;
    /// where and when the light paths of a `ptracer` scene leave the medium: a map of resU x resV cells on every face of the medium shape's
    /// boundary (mer_render_exitance: a grid of the reference's `irradiancemeter` probes on the shape), width x height x spp paths on one device
    struct Exitance {
        int boundary = 0, faces = 6, resU = 1, resV = 1;
        int frames = 1; float tMin = 0.0f, tBin = 0.0f, cosMin = 0.0f;   ///< a steady map: frames 1, tBin 0
        std::vector<double> wavenumbers;        ///< the frequency-domain form: not empty; sums then are [n_freq][2][faces][resV][resU][3]
        double cellArea[6];                     ///< per face: cube u-extent x v-extent / (resU x resV); sphere 4 pi r^2 / (resU x resV)
        std::vector<double> sums;               ///< raw sums [frames][faces][resV][resU][3]
        double totals[16];                      ///< paths, escaped x 3, missed x 3, ended, late x 3, rejected x 3, exits binned, 0 (mer_exitance_read)
        /// sums / (paths x cell area [x tBin for a timed map]), float32 [frames][faces][resV][resU][3]
        std::vector<float> exitance() const;
    };
    /// frames = 1 and tBin = 0: the steady map.  The window is the caller's; the scene's film is not read
    Exitance renderExitance(const Scene &scene, int device, const int res[2], int frames, float tMin, float tBin, float cosMin, int spp, unsigned long long seed) const;
    /// the frequency-domain form (mer_exitance_fd_create): the one exit of a path as w (cos, sin)(k l) per wavenumber; no window
    Exitance renderExitance(const Scene &scene, int device, const int res[2], const std::vector<double> &wavenumbers, float cosMin, int spp, unsigned long long seed) const;
    /// which part of the medium the light that reached a detector travelled through: the absorption sensitivity (Jacobian) of a detector on the
    /// boundary of the medium shape, on a grid of res[0] x res[1] x res[2] cells over the shape's bounding box (mer_render_sensitivity: the
    /// detected light paths of a `ptracer` scene are walked a second time and deposit w x length), width x height x spp paths on one device
    struct Sensitivity {
        int res[3]; float bmin[3], bmax[3];
        std::vector<double> sums;               ///< raw sums J [nz][ny][nx][3]
        double totals[16];                      ///< paths, detected weight x 3, dropped x 3, ended, detected paths, weight x length x 3, replay disagreements, 0 x 3 (mer_sensitivity_read)
        /// J / paths, float32 [nz][ny][nx][3]: minus the derivative of the detected signal per path by the cell's sigma_a
        std::vector<float> jacobian() const;
    };
    /// det: the detector (mer.h); its boundary is set to the scene's.  tBin = 0: no gate
    Sensitivity renderSensitivity(const Scene &scene, int device, const int res[3], mer_detector_desc det, int spp, unsigned long long seed) const;
    /// the sensitivity grids of an array of detectors and gates in one render (mer_sensitivity_array_create): one detector is binU x binV raster
    /// cells of det's window, gate g the exits with floor((l - t_min) / t_bin) == g for 0 <= g < gates; scatter: the scattering grids K too
    struct SensitivityArray {
        int res[3]; float bmin[3], bmax[3];
        int gates = 1, ndv = 1, ndu = 1, scatter = 0;
        std::vector<double> sums;               ///< raw sums [1 + scatter][gates][ndv][ndu][nz][ny][nx][3]: J, then K
        std::vector<double> meas;               ///< [gates][ndv][ndu][8]: detected weight x 3, detected paths, w x scattering collisions x 3, 0
        double totals[16];                      ///< as Sensitivity's; [13..15]: w per collision outside the box (mer_sensitivity_read_array)
        /// sums / paths, float32, in the shape of sums
        std::vector<float> jacobian() const;
    };
    SensitivityArray renderSensitivityArray(const Scene &scene, int device, const int res[3], mer_detector_desc det, int binU, int binV, int gates, bool scatter,
                                            int spp, unsigned long long seed) const;
private:
    struct LightPathSession;                    ///< mer_host.cpp: the one-device session the three recorders above share
    /// the medium's grids (density, albedo, index field, signed distance) onto every context of mm, their handles into d; on failure destroys mm and throws
    void uploadMedia(const Scene &scene, mer_multi *mm, mer_scene_desc &d, int layout) const;
};

class Scene : public ConfigurableObject {
public:
    const char *getClassName() const override { return "Scene"; }
    void addChild(const std::string &name, ObjRef child) override;
    void configure() override;
    std::shared_ptr<Integrator> integrator; std::shared_ptr<Sensor> sensor;
    std::vector<std::shared_ptr<Shape>> shapes; std::vector<std::shared_ptr<Emitter>> emitters;
    std::vector<std::shared_ptr<Medium>> media;
    mutable std::vector<mer_emitter> emitterList;       // storage behind mer_scene_desc.emitters (Integrator::flatten)
};

/// PluginManager::createObject (src/libcore/plugin.cpp:180-196): plugin found by its short name = XML `type`
ObjRef createObject(const std::string &tag, const Properties &props, const std::string &baseDir);

/// SceneHandler: parse a scene file; `defines` are the -D key=value substitutions for $key
std::shared_ptr<Scene> loadScene(const std::string &path, const std::map<std::string, std::string> &defines);
std::shared_ptr<Scene> loadSceneFromString(const std::string &xml, const std::map<std::string, std::string> &defines, const std::string &baseDir);

/// film [h][w][frames*3+2] -> developed RGB [frames][h][w][3] (HDRFilm::develop: divide by the weight channel)
std::vector<float> develop(const std::vector<float> &film, int w, int h, int frames = 1);
void writeNpy(const std::string &path, const float *data, int h, int w, int c);
/// float32 of any shape (`mer_render --fluence --time-resolved`: [frames][nz][ny][nx][3])
void writeNpy(const std::string &path, const float *data, const std::vector<int> &shape);
void writePfm(const std::string &path, const float *rgb, int h, int w);
/// VOL version 3 (src/volume/gridvolume.cpp:108-198), float32: data [nz][ny][nx][channels], the box the first and last nodes lie on
void writeVol(const std::string &path, const float *data, int nx, int ny, int nz, int channels, const float aabbMin[3], const float aabbMax[3]);
/// `mer_render --fluence=NX,NY,NZ`: three counts between 1 and 1024, at most 2^27 cells; false for anything else
bool parseFluenceRes(const std::string &value, int res[3]);
/// `mer_render --exitance=NU,NV`: two counts between 1 and 4096; false for anything else
bool parseExitanceRes(const std::string &value, int res[2]);
/// `mer_render --frequencies=K1[,K2,...]`: 1 ... MER_MAX_FREQUENCIES comma-separated wavenumbers, each finite and at least 0.  0: parsed;
/// 1: the list is empty or an entry is no number; 2: more than MER_MAX_FREQUENCIES entries; 3: an entry is negative or not finite
int parseFrequencies(const std::string &value, std::vector<double> &k);
/// `mer_render --detector=FACE,NU,NV,IU0,IU1,IV0,IV1`: a face 0 ... 5, two counts between 1 and 4096 and a window 0 <= IU0 < IU1 <= NU,
/// 0 <= IV0 < IV1 <= NV, into the face, res and window fields of det; false for anything else
bool parseDetector(const std::string &value, mer_detector_desc &det);
/// OpenEXR 2 scan-line file, uncompressed, three float32 channels B, G, R (what HDRFilm::develop writes through OpenEXR,
/// src/films/hdrfilm.cpp:527; no OpenEXR library is needed for this subset)
void writeExr(const std::string &path, const float *rgb, int h, int w);
/// the image of an `envmap` emitter: a `.pfm` or an uncompressed scan-line OpenEXR file with float32 or half R, G, B channels -> float [h][w][3]
std::vector<float> readEnvmapImage(const std::string &path, int &w, int &h);

}  // namespace merhost

extern "C" {
/* C entry points of libmer_host.so for non-C++ callers (tests): return 0 / 1, message via merhost_last_error() */
const char *merhost_last_error(void);
/* merhost::readEnvmapImage: *w, *h of the file; out = float[h][w][3] when not NULL (query the size first) */
int merhost_read_envmap_image(const char *path, int32_t *w, int32_t *h, float *out);
/* parse + validate only: fills the flat scene (volumes = 0 handles) and width/height/spp; out->emitters (several point or area emitters)
   points to storage of the library that stays valid until the next merhost_flatten_xml call */
int merhost_flatten_xml(const char *path, const char *defines /* "k=v;k=v" */, mer_scene_desc *out, int32_t *spp);
/* the faces of the scene's `obj` medium shape: counts always; vertices (xyz) / triangles (3 indices) when the pointers are not NULL */
int merhost_obj_mesh(const char *path, const char *defines, int64_t *n_vertices, int64_t *n_triangles, float *vertices, int32_t *triangles);
/* flatten as `mer_render --mesh-sdf[=N]` would (n = 0: no N given): the scene with boundary = sdf, and the grid the distance is built on */
int merhost_flatten_xml_mesh_sdf(const char *path, const char *defines, int32_t n, mer_scene_desc *out, mer_grid_desc *grid);
/* parse, upload, render on `device`; film_host = float[h][w][5] of the scene's film size (query with flatten first) */
int merhost_render_xml(const char *path, const char *defines, int32_t device, int32_t spp, uint64_t seed, int32_t layout, float *film_host);
/* the same on n devices (a device may be listed twice): shard_mode = MER_SHARD_SAMPLES | MER_SHARD_TILES */
int merhost_render_xml_multi(const char *path, const char *defines, const int32_t *devices, int32_t n, int32_t shard_mode, int32_t spp, uint64_t seed, int32_t layout,
                             float *film_host);
}
