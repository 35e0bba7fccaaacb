// slam_driver.hpp -- the host-side step scheduler around the kernels.
//
// Two classes with the reference's public surfaces and observable behaviour, written from scratch around this library:
//   PoseTraceT          <->  PoseTrace          (src/common/pose_trace.hpp:28-124)
//   OccupancyGridSLAMT  <->  OccupancyGridSLAM  (src/slam/slam.hpp:21-70), LCM subscriptions replaced by plain handler calls
//                                                and lcm_.publish by three callbacks
// Design notes (what differs from the reference's implementation while giving the same answers):
//   * the trace remembers whether its time stamps ascend; if so poseAt() finds the bracketing samples by bisection
//     (proof of equality with the first-match scan below), otherwise it scans;
//   * one accessor names the trace a mode takes its poses from, so "is there a pose for this scan" is written once;
//   * queued scans live in a ring that reuses its slots (a 10 Hz lidar never makes it grow past a handful);
//   * an iteration is by default the fused two-launch step of DESIGN.md section 5 (filter begin; filter end + map update +
//     fetch of the next queued scan in one launch); setFusedStep(false) gives the call-by-call order.
// Threads: like the reference, handlers and runSLAMIteration() must be called under one lock (slam.cpp holds dataMutex_).
#ifndef BOTLAB_SLAM_DRIVER_HPP
#define BOTLAB_SLAM_DRIVER_HPP

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <iostream>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "beam_model.hpp"
#include "range_table.hpp"
#include "clearance_grid.hpp"
#include "botlab_dropin.hpp"
#include "likelihood_field.hpp"
#include "loop_closer.hpp"
#include "map_rebuild.hpp"
#include "pose_graph.hpp"
#include "scan_matcher.hpp"

namespace botlab_hip {

namespace slam_detail {

const double kTwoPi = 2.0 * M_PI;

// An angle that left [-pi, pi] by less than a turn comes back by one turn (what angle_diff / angle_sum do to their
// result, src/common/angle_functions.hpp:78-87, 128-138).
inline double one_turn_back(double a)
{
    if (std::fabs(a) <= M_PI) return a;
    return a > 0 ? a - kTwoPi : a + kTwoPi;
}

// wrap_to_pi of angle_functions.hpp:12-24 on a float: repeated float additions of the double constant.
inline float wrap_pi(float a)
{
    if (a < -M_PI) { do a += kTwoPi; while (a < -M_PI); }
    else if (a > M_PI) { do a -= kTwoPi; while (a > M_PI); }
    return a;
}

template <class Pose>
inline Pose pose_of(int64_t utime, float x, float y, float theta)
{
    Pose p;
    p.utime = utime; p.x = x; p.y = y; p.theta = theta;
    return p;
}

// Pose between two samples, linear in time (src/common/interpolation.hpp:23-50): float differences, double steps, the
// heading along the shorter arc.  Samples with one time stamp give the later one.
template <class Pose>
inline Pose between(const Pose& a, const Pose& b, int64_t t)
{
    if (a.utime == b.utime) { Pose p = b; p.utime = t; return p; }
    const double s = static_cast<double>(t - a.utime) / static_cast<double>(b.utime - a.utime);
    const double turn = one_turn_back(static_cast<double>(b.theta) - static_cast<double>(a.theta)) * s;
    return pose_of<Pose>(t, static_cast<float>(a.x + (b.x - a.x) * s), static_cast<float>(a.y + (b.y - a.y) * s),
                         static_cast<float>(one_turn_back(static_cast<double>(a.theta) + turn)));
}

// A pose expressed in a frame that is rotated by f.theta and shifted by (f.x, f.y) -- float arithmetic throughout
// (pose_trace.cpp:117-128 uses the float overloads of cos / sin).
template <class Pose>
inline Pose into_frame(const Pose& p, const Pose& f)
{
    const float c = std::cos(f.theta), s = std::sin(f.theta);
    return pose_of<Pose>(p.utime, (p.x * c - p.y * s) + f.x, (p.x * s + p.y * c) + f.y, wrap_pi(p.theta + f.theta));
}

}  // namespace slam_detail

// ---------------------------------------------------------------- PoseTrace
template <class Pose>
class PoseTraceT {
public:
    typedef typename std::vector<Pose>::const_iterator const_iterator;

    PoseTraceT() : frame_(slam_detail::pose_of<Pose>(0, 0.0f, 0.0f, 0.0f)), ascending_(true) {}

    // Samples arrive in the source's frame and are stored in the reference frame (pose_trace.hpp:19-27).
    void addPose(const Pose& pose)
    {
        const Pose placed = slam_detail::into_frame(pose, frame_);
        if (!samples_.empty() && placed.utime < samples_.back().utime) ascending_ = false;
        samples_.push_back(placed);
    }

    // Drops every sample older than `time`, wherever it sits; the others keep their order.  Returns how many went.
    int eraseTraceUntil(int64_t time)
    {
        std::size_t kept = 0;
        for (std::size_t i = 0; i < samples_.size(); ++i)
            if (!(samples_[i].utime < time)) {
                if (kept != i) samples_[kept] = samples_[i];
                ++kept;
            }
        const int dropped = static_cast<int>(samples_.size() - kept);
        samples_.resize(kept);
        if (dropped) recheckOrder();
        return dropped;
    }

    // Pose at `time`: interpolated inside the trace, the nearest end outside it (with a complaint, never extrapolated),
    // the zero pose for an empty trace or when no neighbouring pair brackets the time (possible only in a trace whose
    // stamps do not ascend).
    Pose poseAt(int64_t time) const
    {
        const Pose nothing = slam_detail::pose_of<Pose>(0, 0.0f, 0.0f, 0.0f);
        if (samples_.empty()) {
            std::cerr << "PoseTrace::poseAt(" << time << "): the trace is empty\n";
            return nothing;
        }
        if (time < samples_.front().utime || time > samples_.back().utime) {
            const Pose& end = time < samples_.front().utime ? samples_.front() : samples_.back();
            std::cerr << "PoseTrace::poseAt(" << time << "): outside the trace, answering with the sample at " << end.utime << "\n";
            return end;
        }
        const std::size_t hit = ascending_ ? bracketByBisection(time) : bracketByScan(time);
        return hit ? slam_detail::between(samples_[hit - 1], samples_[hit], time) : nothing;
    }

    bool containsPoseAtTime(int64_t time) const
    {
        return !samples_.empty() && !(time < samples_.front().utime) && !(samples_.back().utime < time);
    }

    // Chooses the frame in which the FIRST sample of the trace (the origin if there is none) becomes the given pose; every
    // stored sample moves there, later ones follow on arrival.  A second call composes with the first, as documented for
    // the reference (pose_trace.hpp:76-90).  Rotation of the offset in double, the stored transform in float
    // (pose_trace.cpp:82-114).
    void setReferencePose(const Pose& initialInReferenceFrame)
    {
        float x0 = 0.0f, y0 = 0.0f, th0 = 0.0f;
        if (!samples_.empty()) { x0 = samples_.front().x; y0 = samples_.front().y; th0 = samples_.front().theta; }
        const double turn = initialInReferenceFrame.theta - th0;
        const double c = std::cos(turn), s = std::sin(turn);
        frame_.x = static_cast<float>(initialInReferenceFrame.x - (x0 * c - y0 * s));
        frame_.y = static_cast<float>(initialInReferenceFrame.y - (x0 * s + y0 * c));
        frame_.theta = static_cast<float>(turn);
        for (std::size_t i = 0; i < samples_.size(); ++i) samples_[i] = slam_detail::into_frame(samples_[i], frame_);
    }

    Pose getFrameTransform() const { return frame_; }
    void clear() { samples_.clear(); ascending_ = true; }

    bool empty() const { return samples_.empty(); }
    std::size_t size() const { return samples_.size(); }
    const_iterator begin() const { return samples_.begin(); }
    const_iterator end() const { return samples_.end(); }
    const Pose& operator[](int index) const { return samples_[index]; }
    const Pose& at(int index) const { return samples_.at(index); }
    const Pose& front() const { return samples_.front(); }
    const Pose& back() const { return samples_.back(); }

private:
    std::vector<Pose> samples_;
    Pose frame_;            // rotation + shift applied to every incoming sample
    bool ascending_;        // utimes never decrease along samples_

    void recheckOrder()
    {
        ascending_ = true;
        for (std::size_t i = 1; i < samples_.size() && ascending_; ++i) ascending_ = !(samples_[i].utime < samples_[i - 1].utime);
    }

    // Index i >= 1 of the FIRST pair (i-1, i) with samples_[i-1].utime <= time <= samples_[i].utime, 0 if there is none.
    // The definition, by scanning (the reference's loop, pose_trace.cpp:57-65):
    std::size_t bracketByScan(int64_t time) const
    {
        for (std::size_t i = 1; i < samples_.size(); ++i)
            if (!(time < samples_[i - 1].utime) && !(samples_[i].utime < time)) return i;
        return 0;
    }
    // Ascending stamps, front <= time <= back (checked by the caller): let i* be the first index >= 1 whose stamp is >= time.
    // Every i in [1, i*) has a stamp < time, so no pair before i* brackets the time; and the stamp at i* - 1 is <= time --
    // for i* = 1 by the caller's check, otherwise because i* - 1 is such an i.  So i* is the scan's answer, equal stamps
    // (several samples with one utime) included.  A single sample has no pair: 0, as the scan.
    std::size_t bracketByBisection(int64_t time) const
    {
        if (samples_.size() < 2) return 0;
        std::size_t lo = 1, hi = samples_.size() - 1;       // the stamp at hi (= back) is >= time
        while (lo < hi) {
            const std::size_t mid = lo + (hi - lo) / 2;
            if (samples_[mid].utime < time) lo = mid + 1; else hi = mid;
        }
        return lo;
    }
};

// ---------------------------------------------------------------- queue of scans waiting for their pose
template <class Scan>
class ScanRing {
public:
    ScanRing() : slots_(8), head_(0), count_(0) {}
    bool empty() const { return count_ == 0; }
    std::size_t size() const { return count_; }
    const Scan& front() const { return slots_[head_]; }
    void push(const Scan& s)
    {
        if (count_ == slots_.size()) grow();
        slots_[(head_ + count_) % slots_.size()] = s;
        ++count_;
    }
    // moves the oldest scan out
    void take(Scan* out)
    {
        std::swap(*out, slots_[head_]);
        head_ = (head_ + 1) % slots_.size();
        --count_;
    }
private:
    std::vector<Scan> slots_;
    std::size_t head_, count_;
    void grow()
    {
        std::vector<Scan> wider(slots_.size() * 2);
        for (std::size_t i = 0; i < count_; ++i) std::swap(wider[i], slots_[(head_ + i) % slots_.size()]);
        slots_.swap(wider);
        head_ = 0;
    }
};

// ---------------------------------------------------------------- OccupancyGridSLAM
template <class Pose, class Lidar, class Odometry, class Particle, class Particles, class GridMsg>
class OccupancyGridSLAMT {
public:
    struct Publisher {                                   // SLAM_POSE, SLAM_PARTICLES, SLAM_MAP (slam.cpp:265-268, 284-289)
        std::function<void(const Pose&)> slamPose;
        std::function<void(const Particles&)> slamParticles;
        std::function<void(const GridMsg&)> slamMap;
    };

    // Same arguments as the reference's constructor (slam.hpp:41-48) with the publisher where the lcm::LCM& stands.
    // 10 m x 10 m grid at 5 cm, 5 m mapping range (slam.cpp:22-24).  Mapping-only and a localization map exclude each other.
    OccupancyGridSLAMT(int numParticles, int8_t hitOddsIncrease, int8_t missOddsDecrease, const Publisher& pub,
                       bool waitForOptitrack, bool mappingOnlyMode = false, bool actionOnlyMode = false,
                       const std::string& localizationOnlyMap = std::string())
        : pf_(numParticles), grid_(10.0f, 10.0f, 0.05f), mapping_(mapRange(), hitOddsIncrease, missOddsDecrease), out_(pub),
          mapHit_(hitOddsIncrease), mapMiss_(missOddsDecrease)
    {
        how_.posesGiven = mappingOnlyMode;
        how_.awaitingFrame = waitForOptitrack;
        if (!mappingOnlyMode && !localizationOnlyMap.empty()) {
            how_.mapKnown = grid_.loadFromFile(localizationOnlyMap);
            how_.mapFromFile = how_.mapKnown;
            how_.odometryOnly = actionOnlyMode;
        }
        const Pose origin = slam_detail::pose_of<Pose>(0, 0.0f, 0.0f, 0.0f);
        start_ = before_ = now_ = odomAtScan_ = origin;
        scan_.utime = 0;
        scan_.num_ranges = 0;
    }

    // ---- inputs.  A scan is kept only if the pose source of this mode already reaches back to its first ray
    // (slam.cpp:90-128); the counter of dropped scans restarts once ten or more were dropped and one is kept.
    void handleLaser(const Lidar& scan)
    {
        const PoseTraceT<Pose>& src = poseSource();
        if (!src.empty() && !(scan.times.front() < src.front().utime)) {
            waiting_.push(scan);
            if (dropped_ >= kDroppedBeforeNotice) {
                std::cout << "OccupancyGridSLAM: poses are arriving, scans are being queued again\n";
                dropped_ = 0;
            }
            return;
        }
        if (++dropped_ == kDroppedBeforeNotice)
            std::cout << "OccupancyGridSLAM: dropping scans, no odometry / pose reaches back to them yet\n";
    }
    void handleOdometry(const Odometry& odometry)
    {
        odom_.addPose(slam_detail::pose_of<Pose>(odometry.utime, odometry.x, odometry.y, odometry.theta));
    }
    void handlePose(const Pose& pose) { truth_.addPose(pose); }
    // the first pose from the tracking system fixes the SLAM frame's start (slam.cpp:150-160)
    void handleOptitrack(const Pose& pose)
    {
        if (!how_.awaitingFrame) return;
        start_ = pose;
        how_.awaitingFrame = false;
    }

    // One launch for "end of updateFilter + updateMap + fetch of the next queued scan" (the default), or the reference's
    // call-by-call order (false).  Results are bit-identical; with the fused step SLAM_POSE / SLAM_PARTICLES of an
    // iteration are published after its map update has been enqueued instead of before.
    void setFusedStep(bool on) { fused_ = on; }

    // (extension) Global localization: in localization-only mode (map from a file, not action-only) the filter is seeded uniformly
    // over the map's free cells instead of around the start pose (the robot's place in the map is not known).  Until the cloud has
    // converged every iteration takes the call-by-call updateFilter path, publishes SLAM_POSE / SLAM_PARTICLES as usual and leaves
    // the map alone (a map extended from an unconverged pose would corrupt the known map).  Converged: the square root of the larger
    // eigenvalue of the particles' weighted x / y covariance <= positionTolerance metres and the heading's circular standard
    // deviation sqrt(-2 ln R) <= headingTolerance radians (ParticleFilterT::spread).  From the first converged iteration on the
    // driver is the plain localization-only driver (fused step, map extended).  Off by default; set before the first iteration.
    void setGlobalLocalization(bool on) { global_ = on; }
    void setGlobalLocalizationThresholds(double positionTolerance, double headingTolerance)
    {
        globalPosTol_ = positionTolerance;
        globalHeadingTol_ = headingTolerance;
    }
    bool globalLocalizationConverged() const { return globalConverged_; }
    // (extension) Global localization by one scan match (ScanMatcherT::matchWide, scan_matcher.hpp): with global localization on, the
    // first scan is matched against the known map over the window given, around the map's middle at heading 0
    // (whole_map_scan_match_params(map) spans the whole map and the whole circle).  An accepted and unique match (ties == 1)
    // starts the filter at that pose (initializeFilterAtPose), and the driver is the plain localization-only driver from the first
    // iteration on (globalLocalizationConverged() is true at once).  Any other outcome seeds uniformly, exactly as without the
    // switch.  Off by default; set before the first iteration.
    void setGlobalLocalizationByScanMatch(const bl_scan_match_wide_params_t& p) { globalMatch_ = true; globalMatchParams_ = p; }
    bool globalLocalizedByScanMatch() const { return globalMatched_; }
    const bl_scan_match_result_t& globalScanMatch() const { return globalMatchResult_; }     // of the first scan (zeros before it)
    // (extension) Global localization judged by the heaviest pose hypothesis (ParticleFilterT::heaviestCluster, bl_pf_clusters)
    // instead of by the whole cloud: while the driver is searching, an iteration counts as converged when the heaviest cluster
    // holds at least minShare of the weight and that cluster's own position and heading deviations -- the two formulas above, on
    // the cluster's moments -- are within the thresholds; a second mode that keeps some weight no longer holds the search up.  Until
    // then SLAM_POSE carries the heaviest cluster's pose (the mean of a multi-modal cloud lies between its modes).  On convergence the
    // filter is started again at the cluster's pose (initializeFilterAtPose, as after an accepted scan match), and from then on the
    // driver is the plain driver.  minShare and the bins of `params` are untuned knobs.  Off by default, and with it off nothing
    // the driver does changes; set before the first iteration.
    void setGlobalLocalizationByCluster(const bl_pf_cluster_params_t& params, double minShare)
    {
        globalCluster_ = true;
        globalClusterParams_ = params;
        globalClusterMinShare_ = minShare;
    }
    const bl_pf_cluster_pose_t& globalCluster() const { return globalClusterPose_; }        // of the last searching iteration (zeros before it)
    // (extension) Kidnapped-robot recovery (ParticleFilterT::enableRecovery, default parameters): in localization-only mode (map from a
    // file, not action-only) recovery is turned on over the map as it stands once the filter is localised -- when it starts from a
    // pose, at the start; with global localization, at the first converged iteration.  From then on every iteration is the
    // call-by-call updateFilter (no fused step: the map update depends on the update's outcome), and an iteration whose update
    // injected particles (the filter no longer fits the measurements) leaves the map alone: a map extended from a wrong pose would
    // hold the filter where it is.  Off by default; set before the first iteration.
    void setKidnapRecovery(bool on) { kidnap_ = on; }
    bool kidnapRecoveryActive() const { return kidnapOn_; }
    int heldMapUpdates() const { return heldMaps_; }          // iterations whose map update recovery held back
    bl_pf_recovery_state_t kidnapRecoveryState() const { return pf_.recoveryState(); }
    // (extension) Adaptive particle count (ParticleFilterT::enableAdaptive, default parameters): the filter is created with the
    // capacity, seeded with all of it (at the start pose, or uniformly with global localization), and from then on every resampling
    // update draws only as many particles as the spread of the posterior needs, down to 200.  Every iteration is then the
    // call-by-call updateFilter.  Composes with global localization and kidnapped-robot recovery.  Off by default; set before the
    // first iteration.
    void setAdaptiveParticles(bool on) { adaptive_ = on; }
    bool adaptiveParticlesActive() const { return adaptiveOn_; }
    bl_pf_adaptive_state_t adaptiveState() const { return pf_.adaptiveState(); }

    // (extension) Correlative scan matching (ScanMatcherT, scan_matcher.hpp): the pose the filter is given as its odometry comes from
    // the scan and the map instead of from the encoders alone.  Every iteration of a mode that runs the filter (not mapping-only)
    // forms a centre -- the last corrected pose composed with the odometry's motion since the last scan (none, if no new odometry
    // arrived) --, matches the scan against the map as it stands around it, and hands the corrected pose to updateFilter /
    // updateFilterActionOnly where the odometry pose went.  A match that is not accepted passes the centre on: dead reckoning from
    // the last corrected pose, which is what an empty map at start-up gives.  The first centre is the start pose.  Every iteration
    // is then the call-by-call updateFilter.  Not combined with global localization (no start pose to chain from: matching stays
    // off there).  Off by default, and with it off nothing the driver does changes; set before the first iteration.
    void setScanMatching(bool on, const bl_scan_match_params_t& p) { matching_ = on; matchParams_ = p; }
    const bl_scan_match_result_t& lastScanMatch() const { return lastMatch_; }
    int scanMatchCount() const { return matches_; }
    // (extension) The match under a motion prior, and a sub-cell corrected pose (ScanMatcherT::matchWithPrior).
    // setScanMatchingPrior: the driver's match becomes matchWithPrior around the same centre -- the prior is centred on the pose
    // dead reckoning gives -- with the coefficients, half_life and want_moments as given (scan_match_prior_from_sigmas forms the
    // coefficients).  setScanMatchingSubCell(true): the corrected pose handed to the filter and chained to the next centre is
    // bl_scanmatch_refined_pose's instead of the whole-cell one; the driver then asks for the moments itself (with no prior set: a
    // zero prior and a half_life of 64).  lastScanMatchMoments(): of the last match that asked for them (zeros before it).
    // correctedPose(): the pose last handed to the filter.  All unset by default, and with them unset the driver's match is
    // bl_scanmatch_match as before; set before the first iteration.
    void setScanMatchingPrior(const bl_scan_match_prior_t& p) { matchPriorSet_ = true; matchPrior_ = p; }
    void setScanMatchingSubCell(bool on) { matchSubCell_ = on; }
    const bl_scan_match_moments_t& lastScanMatchMoments() const { return lastMoments_; }
    const Pose& correctedPose() const { return corrected_; }

    // (extension) Likelihood field (LikelihoodFieldT, likelihood_field.hpp): the filter's update -- and the scan
    // matcher's match, when setScanMatching is on -- read a smoothed field of the map where the map went.  With a map from a file
    // (localization-only) the field is computed once, from the map as loaded; otherwise after every map update, so that the field of
    // iteration k exists before the update of iteration k + 1.  Mapping, seeding, recovery, the global match over the map and the
    // published map keep the real grid.  Every iteration is then the call-by-call updateFilter.  Off by default, and with it off
    // nothing the driver does changes; set before the first iteration.
    void setLikelihoodField(bool on, const bl_lfield_params_t& p) { lfieldOn_ = on; lfieldParams_ = p; }
    bool likelihoodFieldActive() const { return static_cast<bool>(lfield_); }
    const OccupancyGrid& sensorMap() const { return lfield_ ? lfield_->grid() : grid_; }     // what the filter's update reads
    // (extension) Beam model (BeamModelT, beam_model.hpp): every localisation update -- the searching ones of global
    // localization and the ones under recovery included, not the action-only mode -- is followed by bl_beam_reweigh_pf against the
    // real map and the same scan, and the pose of the iteration is the beam-weighted one.  The filter's own update is unchanged; every
    // iteration is then the call-by-call updateFilter.  The recovery tracker keeps folding the sensor update's mean weight, not the
    // beam units (bl_beam_reweigh_pf).  Every parameter is an untuned knob.  Off by default, and with it off nothing the driver does
    // changes; set before the first iteration.  beamModelActive(): the switch is on and an update has been reweighed.
    void setBeamModel(bool on, const bl_beam_params_t& p = default_beam_params()) { beamOn_ = on; beamParams_ = p; }
    bool beamModelActive() const { return beamOn_ && static_cast<bool>(beam_); }
    // (extension) Range table (RangeTableT, range_table.hpp): with the beam model on and a map from a file
    // (localizationOnlyMap), the reweigh looks the expected ranges up in a table of `headings` headings, built from the map before the
    // first reweigh, instead of casting -- AS LONG AS THE DRIVER HAS NOT UPDATED THE MAP SINCE THE TABLE WAS BUILT.  The driver extends
    // its map in every mode (slam.cpp's mode test is always true), so that holds for the iterations that leave the map alone: all of
    // a global search until it converges, the ones recovery holds back, and the first one otherwise.  From the first map update on the
    // switch is ignored and the reweigh casts (by leaps with setBeamLeapCast, cell by cell without): bringing the table up to date
    // after every scan would cost more than the casts it saves, and a stale table is never read.  In every other mode (no map file, poses given, action only) the switch is ignored altogether.
    // Off by default, and with it off nothing the driver does changes; set before the first iteration.  beamRangeTableBuilds() and
    // beamRangeTableReweighs(): tables built (0 or 1) and reweighs that read one.
    void setBeamRangeTable(bool on, int headings = 256) { beamTableOn_ = on; beamTableHeadings_ = headings; }
    int beamRangeTableBuilds() const { return beamTableBuilds_; }
    int beamRangeTableReweighs() const { return beamTableReweighs_; }
    // (extension) Leap cast (ClearanceGridT, clearance_grid.hpp): with the beam model on, the reweigh that would have
    // cast against the map leaps over a clearance grid of cap `cap` instead, with the cast's results value for value -- on a map that
    // changes with every scan, where the range table cannot serve.  A current range table keeps precedence while it is current.  The
    // grid is built from the map before the first leap reweigh; after every map update from then on it is brought up to date in a
    // box -- the bounding box of the cells of the poses of the last and of this map update (every ray starts between the two),
    // widened by ceil(maxLaserDistance * cellsPerMeter) + 2 -- and whatever else writes the map (rebuildMap, optimizeHistory,
    // closeLoops, closeLoopsByPlace) marks it for a whole build before the next reweigh.  THE CAP IS AN UNTUNED KNOB.  Off by
    // default, and with it off nothing the driver does changes; set before the first iteration.  beamLeapBuilds(),
    // beamLeapUpdates() and beamLeapReweighs(): whole builds, boxed updates and reweighs by leaps; beamLeapGrid(): the grid, or null.
    void setBeamLeapCast(bool on, int cap = 64) { beamLeapOn_ = on; beamLeapCap_ = cap; }
    int beamLeapBuilds() const { return beamLeapBuilds_; }
    int beamLeapUpdates() const { return beamLeapUpdates_; }
    int beamLeapReweighs() const { return beamLeapReweighs_; }
    const ClearanceGridT<Pose, Lidar>* beamLeapGrid() const { return beamLeap_.get(); }
    // (extension) Scan history (ScanHistoryT, map_rebuild.hpp): every iteration that updates the map appends the same
    // scan and the same pose bits to a history of the last `capacity` scans -- in the fused step the pose is read on the device, behind
    // the map update that carries the filter's end.  rebuildMap() writes into the driver's map what sequential map updates of the
    // recorded scans at the recorded poses give from an empty map -- the live map itself while the history still holds every scan --
    // and rebuildMap(poses) the same at corrected poses, one per recorded scan.  optimizeHistory below computes corrected poses
    // (DESIGN.md 4.32); the live mapper is neither read nor changed.  Off by default, and with it off nothing the driver does changes; set before the first iteration.
    void setScanHistory(int capacity) { historyCapacity_ = capacity; }
    ScanHistoryT<Pose, Lidar>* scanHistory() const { return history_.get(); }
    void rebuildMap()
    {
        if (history_ && history_->size() > 0) { history_->rebuild(grid_, mapRange(), mapHit_, mapMiss_, 0, history_->size()); beamLeapStale_ = true; }
    }
    void rebuildMap(const std::vector<Pose>& poses)
    {
        if (history_ && !poses.empty()) { history_->rebuild(grid_, mapRange(), mapHit_, mapMiss_, 0, poses); beamLeapStale_ = true; }
    }
    // (extension) Pose-graph back end on the history (PoseGraphT, pose_graph.hpp): the nodes are the recorded poses
    // (device to device), the chain is made from the nodes with the information chainInfo (xx, xy, yy, xt, yt, tt) on every edge, the
    // loop edges are the caller's (botlab_amd.find_loop_closures makes them on the Python side), all of them in force.  Solves, writes
    // the poses back into the history and calls rebuildMap().  false, and nothing done, without a history of at least two scans.
    // Nothing calls it by itself, and with it never called nothing the driver does changes.  lastPoseGraphResult(): of the last call.
    bool optimizeHistory(const std::vector<bl_posegraph_edge_t>& loops, const double chainInfo[6],
                         const bl_posegraph_params_t& params = poseGraphParams())
    {
        if (!history_ || history_->size() < 2) return false;
        const int n = history_->size();
        PoseGraphT<Pose> graph(n, static_cast<int>(loops.size()), 1);
        graph.setNodesFromLog(history_->device(), 0, n);
        graph.setChainFromNodes(chainInfo);
        graph.setLoops(loops);
        graph.solve(params);
        poseGraphResult_ = graph.results()[0];
        graph.posesToLog(0, history_->device(), 0);
        rebuildMap();
        return true;
    }
    const bl_posegraph_result_t& lastPoseGraphResult() const { return poseGraphResult_; }
    // (extension) Loop closure on the history (LoopCloserT, loop_closer.hpp): find -- every candidate pair, submap, match
    // and edge of the history on the device, the submaps at the map's resolution -- then close -- the candidates gated through the pose
    // graph's subsets (alone-cost, then own chi2, against `gate`), the corrected poses written back -- then rebuildMap().  Returns the
    // number of kept edges; 0, and nothing done, without a history of at least two scans (at most 4096: the pose graph's limit).
    // lastPoseGraphResult() is then the last solve's.  Nothing calls it by itself, and with it never called nothing the driver does
    // changes.  Every parameter is an untuned knob.
    int closeLoops(const bl_loopclose_params_t& params, const double chainInfo[6], double gate = 11.345,
                   const bl_posegraph_params_t& graphParams = poseGraphParams())
    {
        if (!history_ || history_->size() < 2) return 0;
        LoopCloserT<Pose, Lidar> closer(loopCloserSlots(params));
        return closeCandidates(closer.find(*history_, grid_, params), chainInfo, gate, graphParams);
    }
    // (extension) closeLoops with the partners chosen by place recognition (LoopCloserT::findPlaces), for a history
    // whose drift is beyond any radius: find by place, close, rebuildMap().  params.radius is not read.  Off unless called; the place
    // parameters are untuned knobs too.
    int closeLoopsByPlace(const bl_loopclose_params_t& params, const bl_place_params_t& place, const double chainInfo[6], double gate = 11.345,
                          const bl_posegraph_params_t& graphParams = poseGraphParams())
    {
        if (!history_ || history_->size() < 2) return 0;
        LoopCloserT<Pose, Lidar> closer(loopCloserSlots(params));
        return closeCandidates(closer.findPlaces(*history_, grid_, params, place), chainInfo, gate, graphParams);
    }
    // (extension) The seed of the filter's first cloud, for runs that can be repeated (the reference, and the default here, take
    // it from the OS).  Set before the first iteration.
    void setFilterSeed(uint64_t seed) { seeded_ = true; seed_ = seed; }

    // The oldest queued scan can be processed once the pose source covers the time of its first ray (slam.cpp:163-188).
    bool isReadyToUpdate() const
    {
        return !how_.awaitingFrame && !waiting_.empty() && poseSource().containsPoseAtTime(waiting_.front().times.front());
    }

    // slam.cpp:191-207: take the scan and its pose / odometry, start the poses on the first call, then localise and map --
    // unless the scan has 100 ranges or fewer.
    void runSLAMIteration()
    {
        waiting_.take(&scan_);
        const int64_t t_end = scan_.times.back();
        if (how_.posesGiven) { before_ = now_; now_ = truth_.poseAt(t_end); }
        else odomAtScan_ = odom_.poseAt(t_end);
        if (!how_.started) startPoses();
        if (scan_.num_ranges <= kFewestRanges) {
            std::cerr << "OccupancyGridSLAM: scan with only " << scan_.num_ranges << " ranges skipped\n";
            return;
        }
        if (scanMatching()) correctOdometry();
        if (globalSearching()) {                        // global localization, not converged yet: filter only, the map is left alone
            before_ = now_;
            now_ = sense(odomAtScan_);
            if (globalCluster_) { searchByCluster(); return; }
            announce();
            globalConverged_ = spreadConverged();
            if (globalConverged_) {
                startRecovery();
                extendMap(false);                       // the first converged iteration extends the map, as every later one does
            }
            return;
        }
        if (kidnapOn_) {                                // recovery on: the map only from an update that did not inject
            before_ = now_;
            now_ = sense(filterOdometry());
            announce();
            if (pf_.recoveryState().p_inject > 0.0) ++heldMaps_;
            else extendMap(false);
            return;
        }
        const bool riding = localize();
        extendMap(riding);
    }

    // ---- inspection (tests)
    const OccupancyGrid& map() const { return grid_; }
    Pose currentPose() const { return now_; }
    int numIgnoredScans() const { return dropped_; }
    std::size_t queuedScans() const { return waiting_.size(); }
    int mapUpdateCount() const { return mapsMade_; }

private:
    enum { kDroppedBeforeNotice = 10, kFewestRanges = 100, kMapEvery = 5 };

    // what closeLoops and closeLoopsByPlace share: a handle with a slot per query, and close + rebuildMap on the candidates found
    int loopCloserSlots(const bl_loopclose_params_t& params) const
    {
        const int n = history_->size();
        const int queries = params.stride >= 1 ? (n + params.stride - 1) / params.stride : 1;
        return queries < BL_LC_MAX_CANDIDATES ? queries : BL_LC_MAX_CANDIDATES;
    }
    int closeCandidates(const std::vector<bl_posegraph_edge_t>& candidates, const double chainInfo[6], double gate,
                        const bl_posegraph_params_t& graphParams)
    {
        PoseGraphT<Pose> graph(history_->size(), static_cast<int>(candidates.size()), static_cast<int>(candidates.size()) + 1);
        const LoopCloseOutcome outcome = LoopCloserT<Pose, Lidar>::close(*history_, graph, candidates, chainInfo, gate, graphParams);
        poseGraphResult_ = outcome.result;
        rebuildMap();
        return static_cast<int>(outcome.kept.size());
    }

    // What the four modes of slam.hpp:72-78 differ in:  mapping-only = posesGiven;  localization-only = mapKnown from a file;
    // action-only = that + odometryOnly;  full SLAM = none of them (mapKnown turns true with the first map update).
    struct How {
        bool posesGiven, odometryOnly, mapKnown, awaitingFrame, started, mapFromFile;
        How() : posesGiven(false), odometryOnly(false), mapKnown(false), awaitingFrame(false), started(false), mapFromFile(false) {}
    };

    How how_;
    PoseTraceT<Pose> truth_, odom_;
    ScanRing<Lidar> waiting_;
    Lidar scan_;                       // the scan of the running iteration
    Pose odomAtScan_;                  // odometry at its last ray
    Pose start_, before_, now_;        // SLAM frame start; pose estimate of the previous / this iteration
    ParticleFilterT<Pose, Lidar, Particle, Particles> pf_;
    OccupancyGrid grid_;
    MappingT<Pose, Lidar> mapping_;
    Publisher out_;
    int dropped_ = 0, mapsMade_ = 0;
    bool fused_ = true;
    // global localization: switch, convergence thresholds (defaults: 0.2 m, 0.3 rad -- more than twice the steady spread of a
    // filter started at the true pose, 0.025 m / 0.10 rad, measured in tests/test_global_init_model_cpu.py), state
    bool global_ = false, globalConverged_ = false;
    double globalPosTol_ = 0.2, globalHeadingTol_ = 0.3;
    // global localization by one scan match: switch and window, whether it placed the filter, the match itself
    bool globalMatch_ = false, globalMatched_ = false;
    bl_scan_match_wide_params_t globalMatchParams_ = bl_scan_match_wide_params_t();
    bl_scan_match_result_t globalMatchResult_ = bl_scan_match_result_t();
    // global localization by the heaviest cluster: switch, bins, the share it must hold, the last searching iteration's cluster
    bool globalCluster_ = false;
    bl_pf_cluster_params_t globalClusterParams_ = bl_pf_cluster_params_t();
    double globalClusterMinShare_ = 0.0;
    bl_pf_cluster_pose_t globalClusterPose_ = bl_pf_cluster_pose_t();
    bool kidnap_ = false, kidnapOn_ = false;     // kidnapped-robot recovery: switch, turned on
    int heldMaps_ = 0;
    bool adaptive_ = false, adaptiveOn_ = false; // adaptive particle count: switch, turned on

    // correlative scan matching: switch and window; the matcher (made on first use); the pose last handed to the filter and the
    // odometry it was formed at; the last match
    bool matching_ = false;
    bl_scan_match_params_t matchParams_ = default_scan_match_params();
    std::unique_ptr<ScanMatcherT<Pose, Lidar> > matcher_;
    bool matchStarted_ = false;
    Pose corrected_, odomAtMatch_;
    bl_scan_match_result_t lastMatch_ = bl_scan_match_result_t();
    int matches_ = 0;
    // the match under a prior: switch and prior; sub-cell switch; the moments of the last match that asked for them
    bool matchPriorSet_ = false, matchSubCell_ = false;
    bl_scan_match_prior_t matchPrior_ = bl_scan_match_prior_t();
    bl_scan_match_moments_t lastMoments_ = bl_scan_match_moments_t();
    // likelihood field: switch and parameters; the field (made when the poses start); the seed of the first cloud, if given
    bool lfieldOn_ = false;
    bl_lfield_params_t lfieldParams_ = default_lfield_params();
    std::unique_ptr<LikelihoodFieldT> lfield_;
    bool seeded_ = false;
    uint64_t seed_ = 0;
    // beam model: switch and parameters; the model (made on first use)
    bool beamOn_ = false;
    bl_beam_params_t beamParams_ = default_beam_params();
    std::unique_ptr<BeamModelT<Pose, Lidar> > beam_;
    // range table: switch and headings; the table (built on first use); the two counters
    bool beamTableOn_ = false;
    int beamTableHeadings_ = 256;
    std::unique_ptr<RangeTableT<Pose, Lidar> > beamTable_;
    int beamTableBuilds_ = 0, beamTableReweighs_ = 0;
    // leap cast: switch and cap; the grid (made on first use); stale: a whole build is due before the next reweigh; the pose of the
    // last map update; the three counters
    bool beamLeapOn_ = false, beamLeapStale_ = true, beamLeapPoseSet_ = false;
    int beamLeapCap_ = 64;
    std::unique_ptr<ClearanceGridT<Pose, Lidar> > beamLeap_;
    Pose beamLeapPose_;
    int beamLeapBuilds_ = 0, beamLeapUpdates_ = 0, beamLeapReweighs_ = 0;
    // scan history: capacity (0: off); the history (made at the first map update); what the mapper was made with
    int historyCapacity_ = 0;
    std::unique_ptr<ScanHistoryT<Pose, Lidar> > history_;
    bl_posegraph_result_t poseGraphResult_ = bl_posegraph_result_t();
    int8_t mapHit_, mapMiss_;
    static float mapRange() { return 5.0f; }               // slam.cpp:24

    // the filter's update from `odometry` and, with the beam model on, its weights replaced by the beam model's
    Pose sense(const Pose& odometry)
    {
        Pose p = pf_.updateFilter(odometry, scan_, sensorMap());
        if (!beamOn_) return p;
        if (!beam_) beam_.reset(new BeamModelT<Pose, Lidar>(beamParams_));
        const int64_t t = p.utime;
        if (beamTableCurrent()) { p = pf_.reweighBeamTable(*beam_, *beamTable_, scan_); ++beamTableReweighs_; }
        else if (beamLeapCurrent()) { p = pf_.reweighBeamLeap(*beam_, *beamLeap_, scan_); ++beamLeapReweighs_; }
        else p = pf_.reweighBeam(*beam_, grid_, scan_);
        p.utime = t;
        return p;
    }

    // true when the reweigh leaps: the switch is on; the grid is made here and built whenever a whole build is due
    bool beamLeapCurrent()
    {
        if (!beamLeapOn_) return false;
        if (!beamLeap_) beamLeap_.reset(new ClearanceGridT<Pose, Lidar>(beamLeapCap_));
        if (beamLeapStale_) {
            beamLeap_->build(grid_, beamParams_.occ_min);
            ++beamLeapBuilds_;
            beamLeapStale_ = false;
        }
        return true;
    }

    // after the map update at now_: the built grid brought up to date in the box of the cells the update can have written
    void beamLeapFollow()
    {
        if (!beamLeapOn_) return;
        const Pose last = beamLeapPoseSet_ ? beamLeapPose_ : now_;
        beamLeapPose_ = now_;
        beamLeapPoseSet_ = true;
        if (!beamLeap_ || beamLeapStale_) return;
        const double cpm = grid_.cellsPerMeter(), ox = grid_.originInGlobalFrame().x, oy = grid_.originInGlobalFrame().y;
        const double ax = std::floor((last.x - ox) * cpm), ay = std::floor((last.y - oy) * cpm);
        const double bx = std::floor((now_.x - ox) * cpm), by = std::floor((now_.y - oy) * cpm);
        const double lim = 1073741824.0;
        if (!(std::fabs(ax) < lim && std::fabs(ay) < lim && std::fabs(bx) < lim && std::fabs(by) < lim)) { beamLeapStale_ = true; return; }
        const int pad = static_cast<int>(std::ceil(static_cast<double>(mapRange()) * cpm)) + 2;
        beamLeap_->update(grid_, static_cast<int>(ax < bx ? ax : bx) - pad, static_cast<int>(ay < by ? ay : by) - pad,
                          static_cast<int>(ax > bx ? ax : bx) + pad, static_cast<int>(ay > by ? ay : by) + pad);
        ++beamLeapUpdates_;
    }

    // true when the reweigh may read the range table: the switch is on, the map came from a file and the driver has not updated it
    // yet (mapsMade_ counts every update, and rebuildMap needs a history that only they fill); the table is built here, once
    bool beamTableCurrent()
    {
        if (!beamTableOn_ || !how_.mapFromFile || mapsMade_ != 0) return false;
        if (!beamTable_) {
            beamTable_.reset(new RangeTableT<Pose, Lidar>(beamTableHeadings_));
            beamTable_->build(*beam_, grid_);
            ++beamTableBuilds_;
        }
        return true;
    }

    bool scanMatching() const { return matching_ && !global_ && !how_.posesGiven; }
    const Pose& filterOdometry() const { return scanMatching() ? corrected_ : odomAtScan_; }

    // The centre of this iteration's match and the match itself.  The odometry's motion since the last match, taken in the odometry
    // frame, is replayed from the last corrected pose: rotated by the difference of the two headings (double arithmetic on the float
    // members, narrowed once).  Odometry that did not move gives the last corrected pose itself.
    void correctOdometry()
    {
        if (!matcher_) matcher_.reset(new ScanMatcherT<Pose, Lidar>());
        if (!matchStarted_) { corrected_ = before_; odomAtMatch_ = odomAtScan_; matchStarted_ = true; }
        const double dx = static_cast<double>(odomAtScan_.x) - static_cast<double>(odomAtMatch_.x);
        const double dy = static_cast<double>(odomAtScan_.y) - static_cast<double>(odomAtMatch_.y);
        const double dth = static_cast<double>(odomAtScan_.theta) - static_cast<double>(odomAtMatch_.theta);
        const double rot = static_cast<double>(corrected_.theta) - static_cast<double>(odomAtMatch_.theta);
        const double c = std::cos(rot), s = std::sin(rot);
        Pose centre = slam_detail::pose_of<Pose>(odomAtScan_.utime, static_cast<float>(corrected_.x + (c * dx - s * dy)),
                                                 static_cast<float>(corrected_.y + (s * dx + c * dy)),
                                                 slam_detail::wrap_pi(static_cast<float>(corrected_.theta + dth)));
        if (matchPriorSet_ || matchSubCell_) {
            bl_scan_match_prior_t prior = matchPrior_;
            if (!matchPriorSet_) prior.half_life = 64;
            if (matchSubCell_) prior.want_moments = 1;
            lastMatch_ = matcher_->matchWithPrior(scan_, centre, sensorMap(), matchParams_, prior, &lastMoments_);
        } else {
            lastMatch_ = matcher_->match(scan_, centre, sensorMap(), matchParams_);
        }
        ++matches_;
        bl_pose_xyt_t to = lastMatch_.pose;
        if (matchSubCell_) {
            const bl_pose_xyt_t c = pose_in(centre);
            bl_scanmatch_refined_pose(&lastMatch_, &lastMoments_, &c, grid_.metersPerCell(), matchParams_.dtheta, &to);
        }
        corrected_ = slam_detail::pose_of<Pose>(odomAtScan_.utime, to.x, to.y, to.theta);
        odomAtMatch_ = odomAtScan_;
    }

    // The first scan against the whole window around the map's middle.  A unique accepted match is the start pose and ends the
    // search before it began; anything else leaves everything as it was.
    void matchOverTheMap()
    {
        if (!matcher_) matcher_.reset(new ScanMatcherT<Pose, Lidar>());
        const PointT<float> o = grid_.originInGlobalFrame();
        const Pose centre = slam_detail::pose_of<Pose>(before_.utime, o.x + 0.5f * grid_.widthInMeters(), o.y + 0.5f * grid_.heightInMeters(), 0.0f);
        globalMatchResult_ = matcher_->matchWide(scan_, centre, grid_, globalMatchParams_);
        if (!globalMatchResult_.accepted || globalMatchResult_.ties != 1) return;
        before_.x = now_.x = globalMatchResult_.pose.x;
        before_.y = now_.y = globalMatchResult_.pose.y;
        before_.theta = now_.theta = globalMatchResult_.pose.theta;
        globalMatched_ = globalConverged_ = true;
    }

    void startRecovery()
    {
        if (!kidnap_ || kidnapOn_ || !how_.mapFromFile || how_.odometryOnly || how_.posesGiven) return;
        pf_.enableRecovery(grid_);
        kidnapOn_ = true;
    }

    bool globalSearching() const { return global_ && how_.mapFromFile && !how_.odometryOnly && !how_.posesGiven && !globalConverged_; }

    // position std (largest principal axis) and heading circular std of the filter's cloud
    bool spreadConverged() const
    {
        const bl_pf_spread_t s = pf_.spread();
        const double h = 0.5 * (s.var_x + s.var_y);
        const double pos = std::sqrt(h + std::sqrt(0.25 * (s.var_x - s.var_y) * (s.var_x - s.var_y) + s.cov_xy * s.cov_xy));
        const double heading = s.theta_resultant > 0.0 ? std::sqrt(-2.0 * std::log(s.theta_resultant)) : HUGE_VAL;
        return pos <= globalPosTol_ && heading <= globalHeadingTol_;
    }

    // One searching iteration under setGlobalLocalizationByCluster, behind its updateFilter: the pose published is the heaviest
    // cluster's; converged on its share and its own two deviations (a resultant of 1 or rounded above it: deviation 0).
    void searchByCluster()
    {
        bl_pf_cluster_pose_t c;
        const bool have = pf_.heaviestCluster(globalClusterParams_, &c);
        if (have) {
            globalClusterPose_ = c;
            now_.x = static_cast<float>(c.mean_x);
            now_.y = static_cast<float>(c.mean_y);
            now_.theta = static_cast<float>(c.theta);
        }
        announce();
        if (!have || !(c.share >= globalClusterMinShare_)) return;
        const double h = 0.5 * (c.var_x + c.var_y);
        const double pos = std::sqrt(h + std::sqrt(0.25 * (c.var_x - c.var_y) * (c.var_x - c.var_y) + c.cov_xy * c.cov_xy));
        const double heading = c.theta_resultant >= 1.0 ? 0.0 : c.theta_resultant > 0.0 ? std::sqrt(-2.0 * std::log(c.theta_resultant)) : HUGE_VAL;
        if (!(pos <= globalPosTol_ && heading <= globalHeadingTol_)) return;
        globalConverged_ = true;
        pf_.initializeFilterAtPose(now_);
        startRecovery();
        extendMap(false);
    }

    const PoseTraceT<Pose>& poseSource() const { return how_.posesGiven ? truth_ : odom_; }

    // slam.cpp:232-250: both poses start at the frame's start pose, stamped with the first scan's first and last ray; the
    // filter is spread around the earlier one.
    void startPoses()
    {
        before_ = now_ = start_;
        before_.utime = scan_.times.front();
        now_.utime = scan_.times.back();
        if (globalSearching() && globalMatch_) matchOverTheMap();
        if (globalSearching()) pf_.initializeFilterUniformly(grid_, 0.0f, before_.utime);
        else {
            if (seeded_) pf_.initializeFilterAtPose(before_, seed_); else pf_.initializeFilterAtPose(before_);
            startRecovery();
        }
        if (lfieldOn_ && !how_.posesGiven) {
            lfield_.reset(new LikelihoodFieldT(lfieldParams_));
            lfield_->compute(grid_);
        }
        if (adaptive_ && !how_.posesGiven) { pf_.enableAdaptive(); adaptiveOn_ = true; }
        how_.started = true;
    }

    void announce()
    {
        const Particles cloud = pf_.particles();
        if (out_.slamPose) out_.slamPose(now_);
        if (out_.slamParticles) out_.slamParticles(cloud);
    }

    // slam.cpp:253-271.  Returns true when the update's end was left to ride in the map launch (fused step).
    bool localize()
    {
        if (how_.posesGiven || !how_.mapKnown) return false;
        before_ = now_;
        if (!how_.odometryOnly && fused_ && !adaptiveOn_ && !scanMatching() && !lfield_ && !beamOn_) {
            pf_.updateFilterBegin(odomAtScan_, scan_, grid_);
            if (!waiting_.empty()) prefetch_scan(waiting_.front());      // the next scan is already queued: it rides along
            return true;
        }
        now_ = how_.odometryOnly ? pf_.updateFilterActionOnly(filterOdometry()) : sense(filterOdometry());
        announce();
        return false;
    }

    // slam.cpp:274-294 (its mode test is always true: the map is extended in every mode); the map goes out with every fifth update.
    bool recording()
    {
        if (historyCapacity_ > 0 && !history_) history_.reset(new ScanHistoryT<Pose, Lidar>(historyCapacity_));
        return static_cast<bool>(history_);
    }

    void extendMap(bool riding)
    {
        if (riding) {
            mapping_.updateMapFinishingFilter(scan_, pf_, odomAtScan_.utime, grid_);
            if (recording()) history_->appendDevicePose(scan_, bl_pf_pose_device_ptr(pf_.device()), odomAtScan_.utime);
            now_ = pf_.poseEstimate();
            announce();
        } else {
            mapping_.updateMap(scan_, now_, grid_);
            if (recording()) history_->append(scan_, now_);
            beamLeapFollow();
        }
        if (lfield_ && !how_.mapFromFile) lfield_->compute(grid_);
        how_.mapKnown = true;
        if (mapsMade_++ % kMapEvery == 0 && out_.slamMap) out_.slamMap(grid_.template toLCM<GridMsg>());
    }
};

}  // namespace botlab_hip

#endif  // BOTLAB_SLAM_DRIVER_HPP
