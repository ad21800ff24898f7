"""Headers catkin would generate from the reference's own interface files, derived at build / test time and never
committed: TEST INFRASTRUCTURE ONLY (used by `make -C oracle ref` and tests/test_integration_patch.py)."""
import os
import re
import sys

REF = "/root/reference"


def generated_headers(dst, ref=REF):
    """What catkin would generate from the reference's own IDL, as plain structs: cfg/RadarModel.cfg -> RadarModelConfig.h,
    msg/*.msg -> <Msg>.h (float32 -> float, uint32 -> uint32_t, T[] -> std::vector<T>, other message types by name)."""
    inc = os.path.join(dst, "radarays_ros")
    os.makedirs(inc, exist_ok=True)
    ctype = {"double": "double", "int": "int", "bool": "bool", "str": "std::string"}
    fields = re.findall(r'gen\.add\(\s*"(\w+)"\s*,\s*(\w+)_t', open(os.path.join(ref, "cfg", "RadarModel.cfg")).read())
    with open(os.path.join(inc, "RadarModelConfig.h"), "w") as f:
        f.write("#pragma once\n#include <string>\nnamespace radarays_ros {\nclass RadarModelConfig {\npublic:\n")
        for name, t in fields:
            f.write("    %s %s;\n" % (ctype[t], name))
        f.write("};\n}\n")
    prim = {"float32": "float", "float64": "double", "uint32": "uint32_t", "int32": "int32_t", "uint8": "uint8_t", "bool": "bool", "string": "std::string"}
    for fn in sorted(os.listdir(os.path.join(ref, "msg"))):
        name = fn[:-4]
        lines = [l.split("#")[0].split() for l in open(os.path.join(ref, "msg", fn)).read().splitlines()]
        lines = [l for l in lines if len(l) >= 2]
        with open(os.path.join(inc, name + ".h"), "w") as f:
            f.write("#pragma once\n#include <cstdint>\n#include <string>\n#include <vector>\n")
            for t, _ in lines:
                base = t.rstrip("[]")
                if base not in prim:
                    f.write("#include <radarays_ros/%s.h>\n" % base)
            f.write("namespace radarays_ros {\nstruct %s {\n" % name)
            for t, field in lines:
                base = t.rstrip("[]")
                c = prim.get(base, base)
                f.write("    %s %s;\n" % ("std::vector<%s>" % c if t.endswith("[]") else c, field))
            f.write("};\n}\n")


if __name__ == "__main__":
    generated_headers(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else REF)
