// registration_information.hpp -- registration information (include/elimaloc_hip_reginfo.h): the C++ face of elm_register_information in
// the shim's types.  The 6 x 6 matrices are in the order [translation; rotation] of the pose's own tangent (t <- t + R v, R <- R Exp(w)),
// which is the order of PoseGraph's edges and priors; they are symmetric, so their storage order does not matter.
#pragma once
#include <vector>

#include "registration.hpp"

// elm_reginfo_config with its defaults: the method's metric, sigma2 = chi2 / dof, the scan's own length scale, nothing dropped
struct RegInfoConfig : elm_reginfo_config {
    RegInfoConfig() { elm_reginfo_config_default(this); }
};

// the matrix to hand to PoseGraph::AddEdges / AddPriors
inline elimaloc::Matrix6d InformationMatrix(const elm_reginfo_result& r) {
    elimaloc::Matrix6d M;
    for (int q = 0; q < 36; ++q) M.data()[q] = r.information[q];
    return M;
}

// One job per scan (sensor frame, PointStruct::pose) at its pose against the map, all in one call: H, the information, the variance
// factor and the eigen-analysis of every job.  The method and the search radius are those of `reg`.
inline std::vector<elm_reginfo_result> RegisterInformation(const std::vector<VoxelHashMap::RadarPointVector>& scans, const VoxelHashMap& map,
                                                           const std::vector<elimaloc::Matrix4d>& poses, const RegistrationConfig& reg,
                                                           const RegInfoConfig& config = RegInfoConfig()) {
    std::vector<elm_reginfo_result> out(scans.size());
    if (scans.empty() || scans.size() != poses.size()) {
        elimaloc::check(scans.empty() ? ELM_OK : ELM_ERR_INVALID, VoxelHashMap::ctx(), "RegisterInformation");
        return out;
    }
    std::vector<double> T(16 * poses.size());
    for (size_t h = 0; h < poses.size(); ++h)
        for (int k = 0; k < 16; ++k) T[16 * h + (size_t)k] = poses[h].data()[k]; // column-major on both sides
    std::vector<elm_scan*> res(scans.size(), nullptr);
    int rc = ELM_OK;
    for (size_t j = 0; j < scans.size() && rc == ELM_OK; ++j) {
        std::vector<float> xyz(3 * scans[j].size() + 1);
        for (size_t i = 0; i < scans[j].size(); ++i)
            for (int k = 0; k < 3; ++k) xyz[3 * i + (size_t)k] = (float)scans[j][i].pose(k);
        rc = elm_scan_upload(VoxelHashMap::ctx(), xyz.data(), scans[j].size(), scans[j].size(), &res[j]);
    }
    const elm_reg_config c = reg.c_struct();
    if (rc == ELM_OK) rc = elm_register_information(VoxelHashMap::ctx(), map.handle(), res.data(), T.data(), (int)scans.size(), &c, &config, out.data());
    for (elm_scan* s : res)
        if (s) elm_scan_destroy(s);
    elimaloc::check(rc, VoxelHashMap::ctx(), "RegisterInformation");
    return out;
}
inline elm_reginfo_result RegisterInformation(const VoxelHashMap::RadarPointVector& scan, const VoxelHashMap& map, const elimaloc::Matrix4d& pose,
                                              const RegistrationConfig& reg, const RegInfoConfig& config = RegInfoConfig()) {
    return RegisterInformation(std::vector<VoxelHashMap::RadarPointVector>(1, scan), map, std::vector<elimaloc::Matrix4d>(1, pose), reg, config)[0];
}
