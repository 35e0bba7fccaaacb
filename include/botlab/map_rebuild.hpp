// map_rebuild.hpp -- scan history and map rebuild over the C ABI (bl_scanlog_*, include/botlab_hip.h, "scan history"): the last
// `capacity` scans kept on the device with their poses, and rebuild(): the map that sequential Mapping::updateMap calls over a window
// of them would leave, byte for byte -- at the recorded poses or at corrected ones, into the same grid or into one of another
// resolution or origin.  OccupancyGridSLAMT::setScanHistory (slam_driver.hpp) records every scan the driver maps.
//
// Corrected poses come from the pose graph (pose_graph.hpp).  C++11.
#ifndef BOTLAB_MAP_REBUILD_HPP
#define BOTLAB_MAP_REBUILD_HPP

#include <cstdint>
#include <vector>

#include "botlab_dropin.hpp"

namespace botlab_hip {

struct LoggedScan { std::vector<float> ranges, thetas; std::vector<int64_t> times; };     // the kept rays of one entry

template <class Pose, class Lidar>
class ScanHistoryT {
public:
    explicit ScanHistoryT(int capacity, int maxRaysPerScan = 8192) : h_(nullptr), maxRays_(maxRaysPerScan)
    {
        check(bl_scanlog_create(default_ctx(), capacity, maxRaysPerScan, &h_), "bl_scanlog_create");
    }
    ~ScanHistoryT() { bl_scanlog_destroy(h_); }
    ScanHistoryT(const ScanHistoryT&) = delete;
    ScanHistoryT& operator=(const ScanHistoryT&) = delete;

    // false (and the history as it was) when the scan keeps more rays than the history holds per scan
    bool append(const Lidar& scan, const Pose& pose)
    {
        bl_lidar_t v = lidar_view(scan);
        bl_pose_xyt_t p = pose_in(pose);
        return bl_scanlog_append(h_, &v, &p) == BL_OK;
    }
    // x, y, theta read from a bl_pose_xyt_t in device memory (ParticleFilterT's bl_pf_pose_device_ptr), stream-ordered; utime given
    bool appendDevicePose(const Lidar& scan, const void* devicePose, int64_t poseUtime)
    {
        bl_lidar_t v = lidar_view(scan);
        return bl_scanlog_append_dev_pose(h_, &v, devicePose, poseUtime) == BL_OK;
    }
    int size() const { return bl_scanlog_size(h_); }

    std::vector<Pose> poses(int first, int count) const
    {
        std::vector<bl_pose_xyt_t> raw(static_cast<std::size_t>(count > 0 ? count : 1));
        if (count > 0) check(bl_scanlog_get_poses(h_, first, count, raw.data()), "bl_scanlog_get_poses");
        std::vector<Pose> out;
        for (int i = 0; i < count; ++i) out.push_back(pose_out<Pose>(raw[static_cast<std::size_t>(i)]));
        return out;
    }
    std::vector<Pose> poses() const { return poses(0, size()); }
    void setPoses(int first, const std::vector<Pose>& poses)
    {
        if (poses.empty()) return;
        const std::vector<bl_pose_xyt_t> raw = rawPoses(poses);
        check(bl_scanlog_set_poses(h_, first, static_cast<int>(raw.size()), raw.data()), "bl_scanlog_set_poses");
    }
    LoggedScan scan(int i) const
    {
        LoggedScan s;
        const std::size_t m = static_cast<std::size_t>(maxRays_);
        s.ranges.resize(m); s.thetas.resize(m); s.times.resize(m);
        int kept = 0;
        check(bl_scanlog_get_scan(h_, i, s.ranges.data(), s.thetas.data(), s.times.data(), &kept), "bl_scanlog_get_scan");
        s.ranges.resize(static_cast<std::size_t>(kept)); s.thetas.resize(static_cast<std::size_t>(kept)); s.times.resize(static_cast<std::size_t>(kept));
        return s;
    }

    // `out` becomes `base` (nullptr: zeros; may be `out` itself) after Mapping(maxLaserDistance, hitOdds, missOdds).updateMap of the
    // entries first .. first + count - 1, in order, at their recorded poses.  prevPose nullptr: the first of them only latches its pose.
    void rebuild(OccupancyGrid& out, float maxLaserDistance, int8_t hitOdds, int8_t missOdds, int first, int count, const Pose* prevPose = nullptr,
                 const OccupancyGrid* base = nullptr)
    {
        run(out, maxLaserDistance, hitOdds, missOdds, first, count, nullptr, prevPose, base);
    }
    // the same at the poses given, one per entry of the window
    void rebuild(OccupancyGrid& out, float maxLaserDistance, int8_t hitOdds, int8_t missOdds, int first, const std::vector<Pose>& poses,
                 const Pose* prevPose = nullptr, const OccupancyGrid* base = nullptr)
    {
        const std::vector<bl_pose_xyt_t> raw = rawPoses(poses);
        run(out, maxLaserDistance, hitOdds, missOdds, first, static_cast<int>(raw.size()), raw.data(), prevPose, base);
    }
    bl_scanlog_stats_t stats() const
    {
        bl_scanlog_stats_t s;
        check(bl_scanlog_last_stats(h_, &s), "bl_scanlog_last_stats");
        return s;
    }
    bl_scanlog* device() const { return h_; }

private:
    bl_scanlog* h_;
    int maxRays_;

    static std::vector<bl_pose_xyt_t> rawPoses(const std::vector<Pose>& poses)
    {
        std::vector<bl_pose_xyt_t> raw;
        for (std::size_t i = 0; i < poses.size(); ++i) raw.push_back(pose_in(poses[i]));
        return raw;
    }
    void run(OccupancyGrid& out, float maxLaserDistance, int8_t hitOdds, int8_t missOdds, int first, int count, const bl_pose_xyt_t* poses,
             const Pose* prevPose, const OccupancyGrid* base)
    {
        bl_pose_xyt_t prev;
        if (prevPose) prev = pose_in(*prevPose);
        const bl_grid* b = base ? base->device() : nullptr;     // (brings base's host edits to the device first)
        check(bl_scanlog_rebuild(h_, first, count, poses, prevPose ? &prev : nullptr, maxLaserDistance, hitOdds, missOdds, b, out.device()),
              "bl_scanlog_rebuild");
        out.markDeviceWritten();
    }
};

}  // namespace botlab_hip

#endif  // BOTLAB_MAP_REBUILD_HPP
