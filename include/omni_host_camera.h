/* omni_host_camera.h -- C entry points of libomni_host_camera.so (omni-swarm_amd/host/host_camera_capi.cpp): the lens model of the key-frame pipeline of
 * omni_host.h -- what the reference's camodocal file (camera_config_path, loop_cam.cpp:31-33) describes and cam->liftProjective applies to every key point
 * (loop_cam.cpp:558-569, :403-407, :289-291).  PINHOLE with distortion coefficients and MEI; the arithmetic is csrc/camera_plan.h's, on the host path and
 * inside the key-frame unit alike.  UNPINNED: camodocal is not vendored, the header's formulas are the specification.  The handle is omni_host.h's
 * omni_pipeline, whoever made it.  Returns as in omni_host.h: 0 on success; after a failure omni_camera_last_error() holds the message (per calling thread). */
#ifndef OMNI_HOST_CAMERA_H
#define OMNI_HOST_CAMERA_H
#include "omni_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct omni_pipeline omni_pipeline;

const char* omni_camera_last_error(void);

/* The lens of every lift of the pipeline: the message's landmarks_2d_norm, the triangulation (on the GPU or on the host, bit for bit the same) and
 * PINHOLE_DEPTH's depth landmarks.  model == NULL: the ideal pinhole (the default).  intrinsics4 = fx fy cx cy (MEI: gamma1 gamma2 u0 v0) of the NETWORK-size
 * image, NULL: the pipeline's stay.  Refused: after the first key frame; an unknown type, a non-finite coefficient, MEI with xi <= 0; any lens in the
 * raw-fisheye mode, whose views are ideal pinholes by construction. */
int omni_pipeline_set_camera_model(omni_pipeline* h, const omni_camera_model* model, const double* intrinsics4);
int omni_pipeline_get_camera_model(omni_pipeline* h, omni_camera_model* model_out, double* intrinsics4_out);

/* The %YAML:1.0 FileStorage text camodocal writes: model_type PINHOLE | MEI (anything else is refused by name), image_width, image_height,
 * distortion_parameters {k1 k2 p1 p2}, projection_parameters {fx fy cx cy | gamma1 gamma2 u0 v0}, mirror_parameters {xi}.  width, height > 0: the
 * intrinsics are scaled to images of that size when the file's image_width x image_height differs (the reference does not scale: a deviation, DESIGN.md
 * section 0.2j); 0: as the file has them.  image_size2_out (may be NULL): the file's image_width, image_height. */
int omni_camera_from_yaml(const char* yaml_text, int width, int height, omni_camera_model* model_out, double* intrinsics4_out, int* image_size2_out);

/* omni_pipeline_create_from_launch (omni_host.h) with the text of the file its camera_config_path names in the place of intrinsics4: lens and intrinsics come
 * from camera_yaml, scaled to the launch file's width x height.  camera_yaml == NULL: the ideal pinhole with a 90 degree field of view, as there. */
omni_pipeline* omni_pipeline_create_from_launch_camera(int device, const char* launch_xml, const char* node_name, const char* args, const char* sp_weights,
                                                       const char* vlad_weights, const char* pca_comp_csv, const char* pca_mean_csv, int precision, int microbatch,
                                                       int pipelines, int storage, int geometry, const char* camera_yaml);

/* The landmarks of one image of a key frame in the database, as its message carries them (ImageDescriptor; direction 0 of a one-direction configuration): *n key
 * points; with out arrays of at least max_n entries and *n <= max_n, landmarks_2d [n][2], landmarks_2d_norm [n][2] -- the lifted floats --, landmarks_3d [n][3]
 * and landmarks_flag [n].  Any out array may be NULL.  For callers that publish the messages themselves and for tests. */
int omni_pipeline_frame_landmarks(omni_pipeline* h, int64_t msg_id, int direction, int max_n, int* n, float* landmarks_2d, float* landmarks_2d_norm, float* landmarks_3d,
                                  uint8_t* landmarks_flag);

#ifdef __cplusplus
}
#endif
#endif /* OMNI_HOST_CAMERA_H */
