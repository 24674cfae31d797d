// camera_model.hpp -- the camera the reference builds from its camodocal file (camera_config_path; loop_cam.cpp:31-33 CameraFactory::generateCameraFromYamlFile)
// as far as LoopCam uses it: cam->liftProjective followed by the division by z (loop_cam.cpp:558-569, :403-407, :289-291).  The arithmetic is
// csrc/camera_plan.h's -- the header the GPU landmark stage runs -- so the host path and the device path lift with the same operations in the same order.
//
// UNPINNED: camodocal is not vendored; camera_plan.h's formulas are the specification for its PINHOLE and MEI models and parity with a camodocal build has
// not been measured.  KANNALA_BRANDT and SCARAMUZZA files are refused by name.
#pragma once
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <string>

#include "../csrc/camera_plan.h"
#include "geometry.hpp"

namespace omni {

struct CameraModel {
    omni_camera_model model = cam::ideal();
    double fx = 300, fy = 300, cx = 300, cy = 240;      // MEI: gamma1, gamma2, u0, v0
    int image_width = 0, image_height = 0;              // the size the file was calibrated at (0: not stated)

    // liftProjective + the division by z of one pixel (any point type with float x, y)
    template <class P> geom::Vec2 lift(const P& p) const {
        double o[2];
        cam::lift(model, fx, fy, cx, cy, p.x, p.y, o);
        return geom::Vec2{o[0], o[1]};
    }
    // the forward model (tests, synthetic data)
    geom::Vec2 project(const geom::Vec3& X) const {
        const double v[3] = {X.x, X.y, X.z};
        double o[2];
        cam::project(model, fx, fy, cx, cy, v, o);
        return geom::Vec2{o[0], o[1]};
    }
    bool ideal() const { return cam::is_ideal(model); }
    void check() const {
        if (const char* why = cam::check(model)) throw std::invalid_argument(why);
        if (!(fx != 0 && fy != 0 && fx == fx && fy == fy)) throw std::invalid_argument("camera model: focal lengths " + std::to_string(fx) + ", " + std::to_string(fy));
    }
    // The intrinsics for images of width x height when the file was calibrated at another size: fx cx by width / image_width, fy cy by height / image_height
    // (the coefficients act on normalised coordinates and stay).  DEVIATION: the reference lifts network-size key points with the file's intrinsics as they
    // are, whatever the size (a quirk of loop_cam.cpp:558-569: correct only when the two sizes agree); INTEGRATION.md tells callers to scale.
    CameraModel scaled(int width, int height) const {
        CameraModel c = *this;
        if (image_width > 0 && image_height > 0 && (image_width != width || image_height != height)) {
            const double sx = (double)width / image_width, sy = (double)height / image_height;
            c.fx = fx * sx; c.cx = cx * sx; c.fy = fy * sy; c.cy = cy * sy;
            c.image_width = width; c.image_height = height;
        }
        return c;
    }

    // The %YAML:1.0 FileStorage text camodocal writes (Camera::writeParametersToYamlFile): model_type, image_width, image_height and the maps
    // distortion_parameters {k1 k2 p1 p2}, projection_parameters {fx fy cx cy | gamma1 gamma2 u0 v0}, mirror_parameters {xi} -- as indented blocks or as
    // {key: value, ...} on one line.  Any model_type but PINHOLE and MEI is refused by name; a missing entry is named.
    static CameraModel from_camodocal_yaml(const std::string& text) {
        std::map<std::string, std::string> kv;              // "key" and "section.key" -> value text
        std::string section;
        auto trim = [](std::string s) {
            const size_t a = s.find_first_not_of(" \t\r"), b = s.find_last_not_of(" \t\r");
            return a == std::string::npos ? std::string() : s.substr(a, b - a + 1);
        };
        auto unquote = [](std::string s) { return s.size() >= 2 && (s.front() == '"' || s.front() == '\'') && s.back() == s.front() ? s.substr(1, s.size() - 2) : s; };
        size_t at = 0;
        while (at < text.size()) {
            size_t end = text.find('\n', at);
            if (end == std::string::npos) end = text.size();
            std::string line = text.substr(at, end - at);
            at = end + 1;
            const size_t hash = line.find('#');
            if (hash != std::string::npos) line.erase(hash);
            const bool indented = !line.empty() && (line[0] == ' ' || line[0] == '\t');
            line = trim(line);
            if (line.empty() || line[0] == '%' || line.compare(0, 3, "---") == 0) continue;
            const size_t colon = line.find(':');
            if (colon == std::string::npos) continue;
            const std::string key = trim(line.substr(0, colon));
            std::string val = trim(line.substr(colon + 1));
            if (!indented) section.clear();
            if (val.empty()) { if (!indented) section = key; continue; }
            if (val[0] == '{') {                            // a flow map on one line
                const size_t close = val.find('}');
                std::string body = val.substr(1, (close == std::string::npos ? val.size() : close) - 1);
                size_t p = 0;
                while (p < body.size()) {
                    size_t q = body.find(',', p);
                    if (q == std::string::npos) q = body.size();
                    const std::string item = body.substr(p, q - p);
                    const size_t c2 = item.find(':');
                    if (c2 != std::string::npos) kv[key + "." + trim(item.substr(0, c2))] = unquote(trim(item.substr(c2 + 1)));
                    p = q + 1;
                }
                continue;
            }
            kv[indented && !section.empty() ? section + "." + key : key] = unquote(val);
        }
        auto need = [&kv](const std::string& k) -> const std::string& {
            const auto it = kv.find(k);
            if (it == kv.end()) throw std::invalid_argument("camodocal file: no " + k);
            return it->second;
        };
        auto num = [&need](const std::string& k) {
            const std::string& s = need(k);
            char* e = nullptr;
            const double v = std::strtod(s.c_str(), &e);
            if (e == s.c_str() || *e) throw std::invalid_argument("camodocal file: " + k + " is not a number: " + s);
            return v;
        };
        CameraModel c;
        const std::string type = need("model_type");
        if (type == "PINHOLE") c.model.type = OMNI_CAMERA_PINHOLE;
        else if (type == "MEI") c.model.type = OMNI_CAMERA_MEI;
        else throw std::invalid_argument("camodocal file: model_type " + type + " is not supported (PINHOLE and MEI are; KANNALA_BRANDT and SCARAMUZZA lifts are not built)");
        c.model.k1 = num("distortion_parameters.k1"); c.model.k2 = num("distortion_parameters.k2");
        c.model.p1 = num("distortion_parameters.p1"); c.model.p2 = num("distortion_parameters.p2");
        if (c.model.type == OMNI_CAMERA_MEI) {
            c.model.xi = num("mirror_parameters.xi");
            c.fx = num("projection_parameters.gamma1"); c.fy = num("projection_parameters.gamma2"); c.cx = num("projection_parameters.u0"); c.cy = num("projection_parameters.v0");
        } else {
            c.model.xi = 0;
            c.fx = num("projection_parameters.fx"); c.fy = num("projection_parameters.fy"); c.cx = num("projection_parameters.cx"); c.cy = num("projection_parameters.cy");
        }
        c.image_width = kv.count("image_width") ? (int)num("image_width") : 0;
        c.image_height = kv.count("image_height") ? (int)num("image_height") : 0;
        c.check();
        return c;
    }
};

}  // namespace omni
