"""KeyframePipeline::Config's raw-fisheye mode alone (tests/cpp/fisheye_config_pin.cpp): what construction refuses -- half a source size, a source size with
configuration 0 or 2, side views that are not width x height, not first_view + 4 views -- and frames_per_keyframe / in_width / in_height / compressed for every
{configuration} x {raw fisheye} x {compressed_images}.  The program is built as a stand-alone executable with -fsanitize=address,undefined and run here; it
constructs no pipeline and links nothing of the GPU library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_checks_run_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "fisheye_config_pin")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-pthread",
                        "-I", os.path.join(ROOT, "omni-swarm_amd", "host"), os.path.join(ROOT, "tests", "cpp", "fisheye_config_pin.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK") and "FAIL" not in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.count("configuration ") == 8                            # 3 configurations x 2 switches, + the raw-fisheye mode x 2
    assert "configuration 1 raw 1 compressed 1: frames 2, in 1280 x 1024, compressed() 1" in r.stdout
    assert "configuration 1 raw 0 compressed 1: frames 8, in 600 x 312, compressed() 0" in r.stdout
