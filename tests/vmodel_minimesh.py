"""A miniature VModelManager over two dicts that stand for the two KV tables (registry: model id -> stored ModelRecord bytes,
vmodels: vmodel id -> stored VModelRecord bytes).  The three writers — updateVModel (VModelManager.java = VMM :137-385),
deleteVModel (:416-470), the tail of PendingTransition.run (:716-767) — are written against the ANSWERS of the two calls
(mmp_vmodels_write_json, mmp_models_refs_json): the mesh parses no stored value and renders none.  Who answers is the caller's
choice: tests/test_vmodel_kat.py plugs in the Python models, tests/test_vmodels_write_gpu.py the device.  Transactions are
all-or-nothing; the copy state (which model loads) is supplied by the script; registerModel / unregisterModel go through
tests/model_register_model.py.  The reads of the status calls use tests/vmodel_model.py's parser, as the read side would."""
from tests import model_refs_model as mr
from tests import model_register_model as mm
from tests import vmodel_model as vm
from tests import vmodel_write_model as wm
from tests.ingest_model import model_bean

INSTANCE = "i-0"


class MeshError(Exception):
    def __init__(self, code, message=""):
        super().__init__(code, message)
        self.code, self.message = code, message


class PythonAnswers:
    """The two calls answered by the sequential models; the registry facts come from the mesh's own stored values."""

    def __init__(self, mesh):
        self.mesh = mesh

    def _registry(self):
        ids = list(self.mesh.registry)
        recs = []
        for k in ids:
            b = model_bean(self.mesh.registry[k], [self.mesh.instance], ["NLCLASSIFIER"], 1)
            recs.append((len(b.loaded), len(b.failed), b.lu, b.type))
        return vm.Registry(ids, recs)

    def write(self, op, flags, strs, old):
        v, r = wm.write_step(op, flags, strs, old, self._registry(), self.mesh.now, self.mesh.age, self.mesh.default_owner)
        return v, r

    def refs(self, flags, last_used, info, old):
        return mr.refs_step(flags, last_used, info, old)

    def committed(self, registry_changes, vmodel_changes):
        pass


class MiniVMesh:
    def __init__(self, now, age, default_owner=b"", answers=None, instance=INSTANCE):
        self.now, self.age, self.default_owner, self.instance = now, age, default_owner, instance
        self.registry, self.vmodels = {}, {}
        self.answers = answers(self) if answers else PythonAnswers(self)

    # ---- the KV store: a transaction is a list of (table, key, value or None) applied together
    def _commit(self, txn):
        reg = {k: v for t, k, v in txn if t == "registry"}
        vms = {k: v for t, k, v in txn if t == "vmodels"}
        for table, changes in ((self.registry, reg), (self.vmodels, vms)):
            for k, v in changes.items():
                if v is None:
                    table.pop(k, None)
                else:
                    table[k] = v
        self.answers.committed(reg, vms)

    # ---- registerModel / unregisterModel (ModelMesh.java:3088-3147, :3181-3203) through the register model
    def register_model(self, model, type_, load_now=False, loads=False):
        flags = mm.LOAD_NOW if load_now else 0
        v, cls, _ = mm.register(flags, 0, (type_, b"", b""), self.registry.get(model, b""), self.now, self.age)
        if cls == mm.CONFLICT:
            raise MeshError("ALREADY_EXISTS")
        if v is not None:
            self._commit([("registry", model, v)])
        if loads:
            self.load(model)

    def unregister_model(self, model):
        _, cls, _ = mm.register(mm.DELETE, 0, (b"", b"", b""), self.registry.get(model, b""), self.now, self.age)
        if cls == mm.REFERENCED:
            raise MeshError("FAILED_PRECONDITION")  # :3188-3191
        if cls == mm.DELETABLE:
            self._commit([("registry", model, None)])

    def load(self, model):
        """The script's copy state: the model is loaded on the one instance (what the instance itself would write)."""
        old = self.registry[model]
        if b'"instanceIds"' not in old:
            sep = b"," if len(old) > 2 else b""
            self._commit([("registry", model, old[:-1] + sep + b'"instanceIds":{"%s":%d}}' % (self.instance.encode(), self.now))])

    def is_loaded(self, model):
        return model in self.registry and b'"instanceIds"' in self.registry[model]

    # ---- decModelRefsInTxn (VMM:475-489) from the answer of a DEC
    def _dec(self, txn, model):
        v, cls, _ = self.answers.refs(0, 0, None, self.registry.get(model, b""))
        if cls == mr.SET:
            txn.append(("registry", model, v))
        elif cls == mr.DELETE:
            txn.append(("registry", model, None))
        elif cls != mr.ENSURE_ABSENT:
            raise MeshError("INTERNAL", "refs class %d" % cls)

    def _decs(self, txn, row, old):
        for k in range(2):
            if row.dec_len[k] >= 0:
                self._dec(txn, old[row.dec_off[k]:row.dec_off[k] + row.dec_len[k]])

    # ---- updateVModel, VMM:137-385
    def set_vmodel(self, vmodel, target, expected_target=b"", owner=b"", type_=b"", auto_delete=False, update_only=False, force=False,
                   load_now=False, sync=False, loads=False):
        stored = self.registry.get(target, b"")
        if type_ and stored and mm.register(0, 0, (type_, b"", b""), stored, self.now, self.age)[1] == mm.CONFLICT:
            raise MeshError("ALREADY_EXISTS")  # VMM:206-214
        flags = (wm.UPDATE_ONLY if update_only else 0) | (wm.FORCE if force else 0) | (wm.LOAD_NOW if load_now else 0) | \
                (wm.TARGET_EXISTS if stored else 0)
        old = self.vmodels.get(vmodel, b"")
        v, row = self.answers.write(wm.SET, flags, (target, expected_target, owner), old)
        if row.cls == wm.NEEDS_TARGET_STATUS:  # VMM:264-265 getStatus(targetModelId) == LOADED
            flags |= wm.TARGET_LOADED if self.is_loaded(target) else wm.TARGET_NOT_LOADED
            v, row = self.answers.write(wm.SET, flags, (target, expected_target, owner), old)
        if row.cls == wm.NOT_FOUND:
            raise MeshError("NOT_FOUND")
        if row.cls == wm.PRECONDITION:
            raise MeshError("FAILED_PRECONDITION")
        if row.cls == wm.OWNER_MISMATCH:
            raise MeshError("ALREADY_EXISTS", 'vmodel %s already exists with different owner "%s"' %
                            (vmodel.decode(), vm.classify(old)[1].owner.decode()))  # VMM:223-225
        if row.cls in wm.RENDERED:
            txn = [("vmodels", vmodel, v)]
            info = (type_, b"", b"") if type_ else None
            tv, tcls, _ = self.answers.refs(mr.INC | (mr.AUTO_DELETE if auto_delete else 0), row.last_used, info, stored)  # VMM:294-302
            if tcls == mr.NOT_FOUND:
                raise MeshError("NOT_FOUND")  # VMM:203-205
            assert tcls in mr.RENDERED
            txn.append(("registry", target, tv))
            self._decs(txn, row, old)
            self._commit(txn)
        elif row.cls != wm.UNCHANGED:
            raise MeshError("INTERNAL", "write class %d" % row.cls)
        if sync and row.flags & wm.IN_TRANSITION:
            self.run_transition(vmodel, loads)
        return self.vmodel_status(vmodel)

    # ---- deleteVModel, VMM:416-470
    def delete_vmodel(self, vmodel, owner=b""):
        old = self.vmodels.get(vmodel, b"")
        _, row = self.answers.write(wm.DELETE, 0, (b"", b"", owner), old)
        if row.cls == wm.DELETED:
            txn = [("vmodels", vmodel, None)]
            self._decs(txn, row, old)
            self._commit(txn)

    # ---- PendingTransition.run, VMM:699-767: the target loads (the script says so), then the record step
    def run_transition(self, vmodel, loads):
        rec = vm.classify(self.vmodels[vmodel])[1]
        frm, to = rec.amid, rec.tmid
        if self.is_loaded(frm):  # VMM:702-703 targetCount > 0: ensureLoaded(toId) blocks until loaded
            if not loads:
                return
            self.load(to)
        old = self.vmodels[vmodel]
        v, row = self.answers.write(wm.COMPLETE, 0, (to, frm, b""), old)
        if row.cls == wm.UPDATED:
            txn = [("vmodels", vmodel, v)]
            self._decs(txn, row, old)
            self._commit(txn)

    # ---- the reads of the reference's assertions
    def vmodel_status(self, vmodel, owner=b""):
        old = self.vmodels.get(vmodel)
        rec = vm.classify(old)[1] if old else None
        if rec is None or (owner and rec.owner != owner):
            return {"status": "NOT_FOUND", "target": "", "active": "", "owner": ""}
        return {"status": "DEFINED" if rec.amid == rec.tmid else "TRANSITIONING", "target": (rec.tmid or b"").decode(),
                "active": (rec.amid or b"").decode(), "owner": (rec.owner or b"").decode(),
                "active_loaded": rec.amid is not None and self.is_loaded(rec.amid)}

    def resolve(self, vmodel):
        return self.vmodel_status(vmodel)["active"]

    def model_found(self, model):
        return model in self.registry


def run_scenario(mesh, steps, after_step=None):
    """Drive a scenario of tests/golden/vmodel_kats.json; every `expect` is asserted.  after_step(mesh, step): the caller's own
    checks behind each step."""
    for st in steps:
        b = lambda k: st.get(k, "").encode()  # noqa: E731
        call, expect, got, error = st["call"], st.get("expect", {}), {}, None
        try:
            if call == "registerModel":
                mesh.register_model(b("model"), b("type"), st.get("load_now", False), st.get("loads", False))
            elif call == "unregisterModel":
                mesh.unregister_model(b("model"))
            elif call == "setVModel":
                got = mesh.set_vmodel(b("vmodel"), b("target"), b("expected_target"), b("owner"), b("type"), st.get("auto_delete", False),
                                      st.get("update_only", False), st.get("force", False), st.get("load_now", False), st.get("sync", False),
                                      st.get("loads", False))
            elif call == "deleteVModel":
                mesh.delete_vmodel(b("vmodel"), b("owner"))
            elif call == "getVModelStatus":
                got = mesh.vmodel_status(b("vmodel"), b("owner"))
            elif call == "getModelStatus":
                got = {"found": mesh.model_found(b("model"))}
            elif call == "resolve":
                got = {"model": mesh.resolve(b("vmodel"))}
            else:
                raise AssertionError(call)
        except MeshError as e:
            error = e
        if "error" in expect:
            assert error is not None and error.code == expect["error"], (st, error)
            if "message" in expect:
                assert error.message == expect["message"], (st, error.message)
        else:
            assert error is None, (st, error)
            for k, want in expect.items():
                assert got[k] == want, (st, k, got)
        if after_step:
            after_step(mesh, st)
